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
 *
 * Orientations (mij_enc_add_coef_oriented; the rules are mjw_tplan_oriented's, mij_host.h).  The load phase is the source's whatever the
 * orientation: tiles of the SOURCE plane.  What is known at compile time is templated -- TR (transpose), NX and NY (the source's x / y axis
 * is mirrored, so odd u / odd v change sign): the position -> zigzag table becomes the transposed one and the signs a constant mask, so
 * every LDS store keeps its constant offset and <0, 0, 0> is the plain kernel.  Only the block geometry is run-time: source block (bx, by)
 * inside the kept extent goes to (ew - 1 - bx | bx, eh - 1 - by | by), swapped when TR, and gets its unit index from the DESTINATION's
 * geometry; a block the trim drops gets u = ~0 and is neither checked nor stored.  The DC predecessor is the previous unit of the component
 * in destination order, mapped back through the same mirrors and swap to a source block index and loaded as before.  The store phase is
 * unchanged: whole 128-byte units are scattered, not pieces.
 *
 * Requantisation (mij_enc_add_coef_requant; the rule is mjw_units_requant's, mij_host.h).  RQ = 1 instances take every coefficient, after the
 * load and the orientation's sign and before the codability check, through y = sgn(x) * ((|x| + (b >> 1)) / b), x = c * a, clamped to
 * +-32767: so codability is judged on the result.  a, b and the constants of the exact division (mjw_requant_magic: one v_mul_hi_u32, no
 * divide and no branch) come from the slot's RqTable, indexed by component class and by the SOURCE position P -- the host has put the destination
 * coefficient's entries there (rq_fill, through the transposition of make_conv_table) -- so every read has a wave-uniform address and a
 * constant offset: scalar loads, no per-lane copy.  The DC predecessor goes through the DC entry before the difference is taken.
 * RQ = 0 instances contain none of this.
 *
 * Windows (mij_enc_add_coef_window; the rules are mjw_tplan_grey's and mjw_tplan_cropped's, mij_host.h).  WIN = 1 instances convert the slots
 * whose destination is a crop of the (oriented) picture, or the grey picture of a colour source.  Both are "which blocks go where", so
 * the tables and signs stay compile-time; what changes is geometry, all run-time: per component class the slot names the kept rectangle
 * of the SOURCE plane in blocks, origin (w_ox, w_oy) and extent (w_ew, w_eh) -- the host has taken the crop back through the transpose,
 * the mirrors and the trim.  A lane whose block lies outside it is dead (u = ~0); one inside mirrors within the rectangle, swaps when TR
 * and takes its unit index from the destination's geometry, which for a grey destination of a colour source is dpm = 1, dh = dv = 1,
 * ny = 1 while the plane keeps the colour source's stride.  The DC predecessor is the destination's previous unit mapped back through
 * swap, mirrors and origin: the first unit of the window predicts from 0 whatever lies left of the cut.  The work list of such a slot
 * names only the tiles that hold a block of the rectangle (enc_coef_convert), and no chroma tile for a grey destination.
 * WIN = 0 instances contain none of this.
 *
 * Restart intervals (mij_enc_set_restart): the DC difference that is checked is the one that will be coded, so the first unit of each component
 * in an MCU whose index in the DESTINATION (after orientation, crop and grey) is a multiple of CoefSlot.ri predicts from 0.  ri is run-time and
 * wave-uniform; ri = 0 skips the test.
 */
#pragma once

#define MIJ_CONV_ROW 68

struct CoefSlot {
	uint64_t coef_off[3], dc_off[3], hi_off[3]; /* bytes into the batch's coefficient arena, per component (DevComp) */
	uint64_t du_off;                            /* bytes into the encoder's unit arena */
	uint32_t mcu_x, mcu_y, lh, lv;              /* the SOURCE's: the planes' geometry */
	uint32_t ncomp, dpm, n_du, slot;            /* n_du: the destination's units; slot: the encoder slot, whose flag an uncodable value raises */
	uint32_t d_mcu_x, d_mcu_y, d_lh, d_lv;      /* the destination's (the source's again for orientation 1) */
	uint32_t ext_x, ext_y;                      /* the source's MCU columns and rows that the trim keeps */
	uint32_t w_ox[2], w_oy[2], w_ew[2], w_eh[2]; /* a windowed slot (win != 0): the kept rectangle of the source plane in blocks, luma and chroma */
	uint32_t win, ri;                           /* win: 1 for a slot the WIN = 1 instances convert; ri: the destination's restart interval in MCUs
	                                               (mij_enc_set_restart), 0: none */
	uint32_t orient, rq;                        /* MIJ_CONV_NX | MIJ_CONV_NY | MIJ_CONV_TR: which template instance converts the slot; rq: 1 + the
	                                               index of the slot's RqTable for a requantising slot (the RQ = 1 instances), 0 for a plain one */
};
enum { MIJ_CONV_NX = 1, MIJ_CONV_NY = 2, MIJ_CONV_TR = 4 };

/* One requantising slot's constants per component class (0 luma, 1 chroma) and source position P: the source step a, the destination
 * step b, and the exact division by b (mjw_requant_magic): m, and h = (b >> 1) + inc, what the magnitude takes before the multiply-high
 * -- the rounding's half and the constant's own increment in one, so that b = 1 needs no case of its own in the kernel. */
struct RqEntry {
	uint32_t m;
	uint8_t a, b, h, pad;
};
struct RqTable {
	RqEntry e[2][64];
};

/* in-block position P -> zigzag index k: the inverse of mij_zigzag_pos (tests/test_transcode_host.py holds the two against each other) */
static constexpr uint8_t k_zigzag_of_pos[64] = {
	0, 10, 3, 21, 2, 9, 20, 35, 1, 19, 8, 34, 4, 11, 22, 36,
	5, 23, 12, 37, 7, 18, 33, 48, 6, 32, 17, 47, 13, 24, 38, 49,
	14, 39, 25, 50, 16, 31, 46, 57, 15, 45, 30, 56, 26, 40, 51, 58,
	27, 52, 41, 59, 29, 44, 55, 62, 28, 54, 43, 61, 42, 53, 60, 63};

/* per source position P = 8 * u + mij_rowslot[v]: the destination's zigzag index ((u, v) -> (v, u) when transposed) and whether the
 * coefficient changes sign (odd u under a mirrored x, odd v under a mirrored y) */
struct ConvTable {
	uint8_t zz[64];
	bool neg[64];
};
/* position P = 8 * u + rowslot[v] -> the position of (v, u): where the transposed block holds the coefficient */
static constexpr int conv_transposed_pos(int P)
{
	constexpr uint8_t rowslot[8] = {0, 4, 2, 5, 1, 6, 3, 7}, row_of_slot[8] = {0, 4, 2, 6, 1, 3, 5, 7};
	return 8 * row_of_slot[P & 7] + rowslot[P >> 3];
}
template <int TR, int NX, int NY>
static constexpr ConvTable make_conv_table()
{
	constexpr uint8_t row_of_slot[8] = {0, 4, 2, 6, 1, 3, 5, 7};
	ConvTable t{};
	for (int P = 0; P < 64; ++P) {
		const int u = P >> 3, v = row_of_slot[P & 7];
		t.zz[P] = k_zigzag_of_pos[TR ? conv_transposed_pos(P) : P];
		t.neg[P] = (NX && (u & 1)) != (NY && (v & 1));
	}
	return t;
}
template <int TR, int NX, int NY>
static constexpr ConvTable k_conv_table = make_conv_table<TR, NX, NY>();

/* The table of a requantising slot for a plan whose tables (zigzag order) go from ya / ca to yb / cb: destination coefficient k sits at
 * source position mij_zigzag_pos[k], or at its transposed position when the slot's instance transposes. */
static inline void rq_fill(RqTable &t, bool tr, const unsigned char *ya, const unsigned char *yb, const unsigned char *ca, const unsigned char *cb)
{
	for (int k = 0; k < 64; ++k) {
		const int P = tr ? conv_transposed_pos(mij_zigzag_pos[k]) : mij_zigzag_pos[k];
		uint32_t yi, ci;
		const uint32_t ym = mjw_requant_magic(yb[k], &yi), cm = mjw_requant_magic(cb[k], &ci);
		t.e[0][P] = RqEntry{ym, ya[k], yb[k], (uint8_t)((yb[k] >> 1) + yi), 0};
		t.e[1][P] = RqEntry{cm, ca[k], cb[k], (uint8_t)((cb[k] >> 1) + ci), 0};
	}
}

/* mjw_units_requant's rule for one value: n = |c * a| + (b >> 1) < 2^24, so the multiply-high of n + inc by m is the exact quotient */
__device__ __forceinline__ int rq_value(int c, const RqEntry &q)
{
	const int x = c * (int)q.a;
	const int y = (int)min(__umulhi((uint32_t)(x < 0 ? -x : x) + q.h, q.m), 32767u);
	return x < 0 ? -y : y;
}

template <int COMPACT, int TR = 0, int NX = 0, int NY = 0, int RQ = 0, int WIN = 0>
__global__ __launch_bounds__(64) void k_coef_units(const CoefSlot *__restrict__ slots, const WorkIdct *__restrict__ work, const uint8_t *__restrict__ coef,
																	uint8_t *__restrict__ du_base, uint32_t *__restrict__ s_flag, const RqTable *__restrict__ rqt)
{
	__shared__ int16_t rows[64 * MIJ_CONV_ROW];
	__shared__ uint32_t unit_of[64];
	const WorkIdct wk = work[blockIdx.x];
	const CoefSlot &s = slots[wk.img]; /* read in place (scalar loads): a copy indexed by c would live in scratch, 184 bytes per lane */
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
	if constexpr (RQ) { /* sign (with the int16 wrap the plain path's cast has), then the new step: the check below sees the result */
		const RqEntry *q = rqt[s.rq - 1u].e[c ? 1 : 0]; /* wave-uniform: scalar loads */
#pragma unroll
		for (int P = 0; P < 64; ++P)
			val[P] = rq_value(k_conv_table<TR, NX, NY>.neg[P] ? (int)(int16_t)-val[P] : val[P], q[P]);
	}
	constexpr bool PLAIN = !TR && !NX && !NY && !WIN; /* orientation 1 and no window: the destination is the source */
	/* the kept extent of the source plane in blocks (a window: a rectangle with an origin), and the destination's geometry for this component */
	const uint32_t ox = WIN ? s.w_ox[c ? 1 : 0] : 0u, oy = WIN ? s.w_oy[c ? 1 : 0] : 0u;
	const uint32_t ew = WIN ? s.w_ew[c ? 1 : 0] : PLAIN ? bw : s.ext_x * h, eh = WIN ? s.w_eh[c ? 1 : 0] : PLAIN ? s.mcu_y * v : s.ext_y * v;
	const uint32_t dh = PLAIN ? h : (c ? 1u : s.d_lh), dv = PLAIN ? v : (c ? 1u : s.d_lv), dmcu_x = PLAIN ? s.mcu_x : s.d_mcu_x;
	const uint32_t sbx = L % bw, sby = L / bw;
	uint32_t u = ~0u;
	if (live && sbx - ox < ew && sby - oy < eh) { /* unsigned: a block left of or above the origin wraps and is out */
		const uint32_t x1 = NX ? ew - 1u - (sbx - ox) : sbx - ox, y1 = NY ? eh - 1u - (sby - oy) : sby - oy;
		const uint32_t bx = TR ? y1 : x1, by = TR ? x1 : y1; /* the block's place in the destination */
		const uint32_t mx = bx / dh, my = by / dv, sx = bx - mx * dh, sy = by - my * dv;
		const uint32_t ny = s.ncomp == 1u ? 1u : s.lh * s.lv; /* ncomp is the destination's: 1 for a grey destination of a colour source */
		u = (my * dmcu_x + mx) * s.dpm + (c ? ny + c - 1u : sy * dh + sx);
		if (u >= s.n_du)
			u = ~0u;
		/* the block whose DC predicts this one's: the destination's previous unit of the component, (px, py) there */
		uint32_t px = 0, py = 0;
		bool has = true;
		if (sx > 0)
			px = bx - 1u, py = by;
		else if (sy > 0)
			px = mx * dh + dh - 1u, py = by - 1u;
		else if (s.ri && (my * dmcu_x + mx) % s.ri == 0u) /* the first MCU of a restart interval of the destination: predicted from 0 */
			has = false;
		else if (mx > 0)
			px = mx * dh - 1u, py = my * dv + dv - 1u;
		else if (my > 0)
			px = dmcu_x * dh - 1u, py = my * dv - 1u;
		else
			has = false;
		int pred = 0;
		if (has) {
			/* back through the swap and the mirrors to the source plane's block index */
			const uint32_t qx = TR ? py : px, qy = TR ? px : py;
			const size_t pb = (size_t)(oy + (NY ? eh - 1u - qy : qy)) * bw + (ox + (NX ? ew - 1u - qx : qx));
			if (COMPACT)
				pred = reinterpret_cast<const int16_t *>(coef + s.dc_off[c])[pb];
			else
				pred = reinterpret_cast<const int16_t *>(coef + s.coef_off[c])[((size_t)(pb >> 6) << 12) + ((size_t)(pb & 63) << 3)];
		}
		if constexpr (RQ)
			pred = rq_value(pred, rqt[s.rq - 1u].e[c ? 1 : 0][0]);
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
		rows[lane * MIJ_CONV_ROW + k_conv_table<TR, NX, NY>.zz[P]] = (int16_t)(!RQ && k_conv_table<TR, NX, NY>.neg[P] ? -val[P] : val[P]);
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
