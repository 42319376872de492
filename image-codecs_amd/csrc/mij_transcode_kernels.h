/*
 * mij_transcode_kernels.h -- lossless transcode on the GPU (mij_enc_add_coef, include/mij.h): a batch slot's quantised coefficient
 * planes, as the decode front ends leave them in HBM, re-ordered into the writer's data units in the encoder's unit arena, where the
 * emission kernels (mij_emit_kernels.h) find them like any other slot's.  Included by mij_runtime.hip.
 *
 * k_coef_units, one wavefront per 64-block plane tile of one component (the work list names slot, component and tile):
 *   load     lane l owns block l of the tile and reads its eight chunks the way the band kernels do -- 16 bytes (int16 planes) or 8 bytes
 *            (compact planes) at (chunk * 64 + l), one coalesced 1 KiB / 512 B access per chunk across the wave; all eight are issued
 *            before the first is used.  Compact planes: the DC comes from the DC array, the 64 escape bytes are read for flagged blocks only.
 *   check    the same pass decides codability: an AC value outside -1023..1023, or a DC difference outside -2047..2047 against the
 *            predecessor's DC (the previous unit of the component in MCU order: one 2-byte load), raises the slot's flag with an atomic OR.
 *            k_emit_count refuses a flagged slot before it packs anything.
 *   reorder  each coefficient goes to its zigzag place in the lane's LDS row (the position -> zigzag index map is a compile-time table:
 *            every store has a constant offset); rows are MIJ_CONV_ROW halfwords apart, 34 dwords, so that the lanes' rows start in
 *            different banks and 8-byte reads stay aligned.
 *   store    eight passes: lanes 8b .. 8b + 7 store the 128 bytes of one unit as eight contiguous 16-byte pieces at the unit's MCU-order
 *            place, eight units per pass.
 * Unit index of block (bx, by) of a component with factors h x v: MCU (bx / h, by / v), sub-block (bx % h, by % v):
 *   u = (my * mcu_x + mx) * dpm + first + sy * h + sx,  first = 0 for luma, ny for Cb, ny + 1 for Cr.
 */
#pragma once

#define MIJ_CONV_ROW 68

struct CoefSlot {
	uint64_t coef_off[3], dc_off[3], hi_off[3]; /* bytes into the batch's coefficient arena, per component (DevComp) */
	uint64_t du_off;                            /* bytes into the encoder's unit arena */
	uint32_t mcu_x, mcu_y, lh, lv;
	uint32_t ncomp, dpm, n_du, slot;            /* slot: the encoder slot, whose flag an uncodable value raises */
};

/* in-block position P -> zigzag index k: the inverse of mij_zigzag_pos (tests/test_transcode_host.py holds the two against each other) */
static constexpr uint8_t k_zigzag_of_pos[64] = {
	0, 10, 3, 21, 2, 9, 20, 35, 1, 19, 8, 34, 4, 11, 22, 36,
	5, 23, 12, 37, 7, 18, 33, 48, 6, 32, 17, 47, 13, 24, 38, 49,
	14, 39, 25, 50, 16, 31, 46, 57, 15, 45, 30, 56, 26, 40, 51, 58,
	27, 52, 41, 59, 29, 44, 55, 62, 28, 54, 43, 61, 42, 53, 60, 63};

template <int COMPACT>
__global__ __launch_bounds__(64) void k_coef_units(const CoefSlot *__restrict__ slots, const WorkIdct *__restrict__ work, const uint8_t *__restrict__ coef,
																	uint8_t *__restrict__ du_base, uint32_t *__restrict__ s_flag)
{
	__shared__ int16_t rows[64 * MIJ_CONV_ROW];
	__shared__ uint32_t unit_of[64];
	const WorkIdct wk = work[blockIdx.x];
	const CoefSlot s = slots[wk.img];
	const uint32_t c = wk.comp, tile = wk.first, lane = threadIdx.x;
	const uint32_t h = c ? 1u : s.lh, v = c ? 1u : s.lv, bw = s.mcu_x * h, nblk = bw * s.mcu_y * v;
	const uint32_t L = tile * 64u + lane;
	const bool live = L < nblk;
	int val[64]; /* the block in position order */
	if (COMPACT) {
		const uint2 *lo = reinterpret_cast<const uint2 *>(coef + s.coef_off[c] + (size_t)tile * 4096);
		uint2 ch[8];
#pragma unroll
		for (int q = 0; q < 8; ++q)
			ch[q] = lo[q * 64 + lane];
		const int dc = reinterpret_cast<const int16_t *>(coef + s.dc_off[c])[L];
#pragma unroll
		for (int q = 0; q < 8; ++q)
#pragma unroll
			for (int j = 0; j < 8; ++j)
				val[8 * q + j] = (int)(int8_t)(((j < 4 ? ch[q].x : ch[q].y) >> (8 * (j & 3))) & 0xFFu);
		if (live && (ch[0].x & 1u)) { /* an escaped block: coefficient = sext8(low byte) + 256 * escape byte (mod 2^16) */
			const uint4 *hi = reinterpret_cast<const uint4 *>(coef + s.hi_off[c] + (size_t)L * 64);
#pragma unroll
			for (int q = 0; q < 4; ++q) {
				const uint4 e = hi[q];
				const uint32_t w[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
				for (int j = 0; j < 16; ++j)
					val[16 * q + j] = (int)(int16_t)(val[16 * q + j] + 256 * (int)(int8_t)((w[j >> 2] >> (8 * (j & 3))) & 0xFFu));
			}
		}
		val[0] = dc;
	} else {
		const uint4 *pl = reinterpret_cast<const uint4 *>(coef + s.coef_off[c] + (size_t)tile * 8192);
		uint4 ch[8];
#pragma unroll
		for (int q = 0; q < 8; ++q)
			ch[q] = pl[q * 64 + lane];
#pragma unroll
		for (int q = 0; q < 8; ++q) {
			const uint32_t w[4] = {ch[q].x, ch[q].y, ch[q].z, ch[q].w};
#pragma unroll
			for (int j = 0; j < 8; ++j)
				val[8 * q + j] = (int)(int16_t)(w[j >> 1] >> (16 * (j & 1)));
		}
	}
	uint32_t u = ~0u;
	if (live) {
		const uint32_t bx = L % bw, by = L / bw, mx = bx / h, my = by / v, sx = bx - mx * h, sy = by - my * v;
		const uint32_t ny = s.ncomp == 1u ? 1u : s.lh * s.lv;
		u = (my * s.mcu_x + mx) * s.dpm + (c ? ny + c - 1u : sy * h + sx);
		if (u >= s.n_du)
			u = ~0u;
		/* the block whose DC predicts this one's */
		long pb = -1;
		if (sx > 0)
			pb = (long)L - 1;
		else if (sy > 0)
			pb = (long)(by - 1u) * bw + (mx * h + h - 1u);
		else if (mx > 0)
			pb = (long)(my * v + v - 1u) * bw + (mx * h - 1u);
		else if (my > 0)
			pb = (long)(my * v - 1u) * bw + (bw - 1u);
		int pred = 0;
		if (pb >= 0) {
			if (COMPACT)
				pred = reinterpret_cast<const int16_t *>(coef + s.dc_off[c])[pb];
			else
				pred = reinterpret_cast<const int16_t *>(coef + s.coef_off[c])[((size_t)(pb >> 6) << 12) + ((size_t)(pb & 63) << 3)];
		}
		bool bad = (uint32_t)(val[0] - pred + 2047) > 4094u;
#pragma unroll
		for (int P = 1; P < 64; ++P)
			bad = bad || (uint32_t)(val[P] + 1023) > 2046u;
		if (bad)
			atomicOr(&s_flag[s.slot], 1u);
	}
	unit_of[lane] = u;
#pragma unroll
	for (int P = 0; P < 64; ++P)
		rows[lane * MIJ_CONV_ROW + k_zigzag_of_pos[P]] = (int16_t)val[P];
	__syncthreads();
#pragma unroll
	for (int i = 0; i < 8; ++i) {
		const uint32_t b = (uint32_t)i * 8u + (lane >> 3), q = lane & 7u, ub = unit_of[b];
		if (ub == ~0u)
			continue;
		const uint2 *r = reinterpret_cast<const uint2 *>(&rows[b * MIJ_CONV_ROW + q * 8u]);
		const uint2 a = r[0], d = r[1];
		*reinterpret_cast<uint4 *>(du_base + s.du_off + (size_t)ub * 128 + q * 16u) = make_uint4(a.x, a.y, d.x, d.y);
	}
}
