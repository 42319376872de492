/*
 * mij_progressive_kernels.h -- progressive emission on the GPU (mij_enc_set_progressive, include/mij.h; the contract is include/mij_host.h,
 * PROGRESSIVE STREAMS: libjpeg's jpeg_simple_progression script and jcphuff.c's semantics).  Included by mij_emit_kernels.h, whose six
 * launches write a progressive slot's stream as they write any other: a SCAN is a segment as a restart interval is.
 *
 * Tiles.  A progressive slot's tile list names (scan, first block, count): EmitTile.first counts units in a DC scan (interleaved: every
 * unit in the writer's order) and blocks of the scan's component in raster order in an AC scan; EmitTile.pad carries the scan in bits 16-19.
 * A scan's first tile has MIJ_TILE_STARTS, its last MIJ_TILE_FILLS (the 7 fill bits) and, when another scan follows, MIJ_TILE_ENDS: the
 * bit offsets restart behind it (k_emit_scan) and the next scan's header -- its DHT segments and SOS, written by k_prog_build, of variable
 * length -- is inserted in byte space where a restart marker would stand (k_emit_stuff, k_emit_write).  The first scan's header follows the
 * frame header inside the slot's header.
 *
 * Lanes.  One wavefront per block, lane k = zigzag k.  prog_tile_setup turns the tile's blocks into unit indices once per tile (the only
 * division); the per-block path has none.  DC scans: lane 0 owns the difference's symbol (first scan, values shifted arithmetically) or the
 * one bit (refinement).  AC scans, prog_ac_block: ballots classify the band's lanes as zero, newly non-zero (N) or, in refinement, already
 * non-zero (C, one correction bit); popcounts over those masks give each N lane its zero run and its ZRLs, and every bit its place under
 * jcphuff.c's buffering rule: correction bits stand behind the next EVENT -- the first ZRL written at a non-zero lane, otherwise the
 * N lane's symbol and sign -- and those behind the block's last N lane are its TAIL.
 *
 * EOB runs.  Stream order is body(A), EOBn, tail(A), tail(B), ... for a run that starts in block A, so A owns the EOBn symbol and every
 * block's bits are contiguous.  A needs the run's length ahead of it: k_prog_flags leaves a byte per block (has an N lane; ends its band
 * without one; tail bits) and a summary per tile, k_prog_runs scans the summaries of each scan in reverse, and prog_tile_setup joins both
 * into each block's role.  The EOBn symbols are counted for the tables, so all this runs in front of k_prog_hist.
 *
 * Forced flushes are sequential and do not run here: a run of 32767 blocks or more, a run with more than 937 correction bits pending and a
 * table K.2 cannot build (no plain table has EOBn codes) raise the slot's flag; k_emit_count refuses the slot and the host writer finishes
 * it from its units (MIJ_ENC_SLOT_HOST_FLUSH).
 *
 * Launches in front of the six, over progressive tiles only and none without a progressive slot: k_prog_flags, k_prog_runs, k_prog_hist,
 * k_prog_build.  Their number grows neither with the slots nor with the scans.
 */
#pragma once

#define MIJ_PROG_SCANS 10
#define MIJ_PROG_HDR 320 /* the stride of the scan headers: a DHT segment of at most 5 + 16 + 256 bytes and an SOS of at most 14 */
#define MIJ_PROG_MAX_RUN 32767u
#define MIJ_PROG_MAX_PENDING 937u

struct ProgScanDef {
	uint8_t comp, ss, se, ah, al, ncomp; /* comp: 0 luma, 1 Cb, 2 Cr (AC scans); ncomp: components in the scan */
};
/* jpeg_simple_progression: [0] three components, [1] grey (its first six entries) */
#define MIJ_PROG_SCRIPT \
	{{{0, 0, 0, 0, 1, 3}, {0, 1, 5, 0, 2, 1}, {2, 1, 63, 0, 1, 1}, {1, 1, 63, 0, 1, 1}, {0, 6, 63, 0, 2, 1}, \
	  {0, 1, 63, 2, 1, 1}, {0, 0, 0, 1, 0, 3}, {2, 1, 63, 1, 0, 1}, {1, 1, 63, 1, 0, 1}, {0, 1, 63, 1, 0, 1}}, \
	 {{0, 0, 0, 0, 1, 1}, {0, 1, 5, 0, 2, 1}, {0, 6, 63, 0, 2, 1}, {0, 1, 63, 2, 1, 1}, {0, 0, 0, 1, 0, 1}, {0, 1, 63, 1, 0, 1}, \
	  {0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}}}
__device__ const ProgScanDef k_prog_script[2][MIJ_PROG_SCANS] = MIJ_PROG_SCRIPT;
static const ProgScanDef k_prog_script_host[2][MIJ_PROG_SCANS] = MIJ_PROG_SCRIPT;

struct ProgSlot {
	uint32_t slot, nscan, grey, lh, lv, mcu_x;
	uint32_t frame_len;                 /* SOI .. SOF2 in the slot's header; the first scan's tables and SOS follow */
	uint32_t tab0;                      /* scan k's tables are entry tab0 + k */
	uint32_t bw[MIJ_PROG_SCANS];        /* block columns of an AC scan's component */
	uint32_t tile0[MIJ_PROG_SCANS + 1]; /* the first tile of each scan, in the tile list */
	uint64_t flag_off[MIJ_PROG_SCANS];  /* an AC scan's block bytes in the flag arena */
};
struct ProgTileSum {
	uint32_t n_has, lead, lead_bits, sum_bits; /* blocks | 1u << 31 when a block has an N lane; the empty blocks in front of the first such; tail bits of those; of all */
};
struct ProgAfter {
	uint32_t len, bits; /* the empty blocks that follow the tile in its scan before one with an N lane, and their tail bits */
};
#define MIJ_PROG_HAS 0x80u
#define MIJ_PROG_OPEN 0x40u /* the block's band does not end in an N lane: it adds one to EOBRUN */

struct ProgLds {
	uint32_t uidx[MIJ_EMIT_TILE]; /* block -> unit */
	uint32_t role[MIJ_EMIT_TILE]; /* the EOB run the block writes (it starts one), 0: none */
	uint32_t ptb[MIJ_EMIT_TILE];  /* inclusive sums of the tail bits */
	uint8_t fl[MIJ_EMIT_TILE];
};

__device__ __forceinline__ uint32_t prog_tile_scan(const EmitTile &tl) { return (tl.pad >> 16) & 15u; }

/* the unit of block b (raster order, bw columns) of component comp: one division */
__device__ __forceinline__ uint32_t prog_block_unit(const ProgSlot &ps, const EmitSlot &s, uint32_t comp, uint32_t bw, uint32_t b)
{
	const uint32_t by = b / bw, bx = b - by * bw;
	if (comp || ps.grey)
		return (by * ps.mcu_x + bx) * s.dpm + (comp ? s.ny + comp - 1u : 0u);
	const uint32_t sx = ps.lh == 2u ? 1u : 0u, sy = ps.lv == 2u ? 1u : 0u;
	return ((by >> sy) * ps.mcu_x + (bx >> sx)) * s.dpm + (by & sy) * ps.lh + (bx & sx);
}

/* the first event lane above `lane`, the last one below: on 64-bit masks */
__device__ __forceinline__ int prog_msb(uint64_t m) { return 63 - __clzll((long long)m); }

/* Per tile, by the whole workgroup (ends in a barrier): unit indices and, for an AC scan whose flags exist (fl != NULL), every block's role.
 * p_flag (k_prog_hist only): raised for a run that libjpeg would flush early. */
__device__ void prog_tile_setup(const ProgSlot &ps, const EmitSlot &s, const EmitTile &tl, uint32_t g, ProgScanDef sc, const uint8_t *__restrict__ fl,
										  const ProgAfter *__restrict__ t_after, uint32_t *__restrict__ p_flag, ProgLds *L)
{
	const uint32_t n = emit_tile_units(tl), scan = prog_tile_scan(tl);
	const int lane = threadIdx.x & 63;
	if (sc.ss == 0) { /* a DC scan: units in order, no runs */
		__syncthreads();
		return;
	}
	const uint8_t *f = fl ? fl + ps.flag_off[scan] + tl.first : nullptr;
	if (threadIdx.x < MIJ_EMIT_TILE) {
		const uint32_t j = threadIdx.x;
		L->uidx[j] = j < n ? prog_block_unit(ps, s, sc.comp, ps.bw[scan], tl.first + j) : 0u;
		L->fl[j] = f && j < n ? f[j] : 0;
		L->role[j] = 0;
	}
	__syncthreads();
	if (!f)
		return;
	uint64_t S0 = 0, S1 = 0, E0 = 0, E1 = 0;
	uint32_t tb0 = 0, tb1 = 0, P0 = 0, P1 = 0;
	if (threadIdx.x < 64) {
		const uint32_t a = L->fl[lane], b = L->fl[lane + 64];
		S0 = __ballot((a & MIJ_PROG_HAS) != 0);
		S1 = __ballot((b & MIJ_PROG_HAS) != 0);
		E0 = __ballot((a & MIJ_PROG_OPEN) != 0);
		E1 = __ballot((b & MIJ_PROG_OPEN) != 0);
		tb0 = a & 63u, tb1 = b & 63u;
		P0 = wave_incl_scan(tb0, lane);
		P1 = __shfl(P0, 63, 64) + wave_incl_scan(tb1, lane);
		L->ptb[lane] = P0;
		L->ptb[lane + 64] = P1;
	}
	__syncthreads();
	if (threadIdx.x < 64) {
		const ProgAfter after = t_after[g];
		const bool prev_open0 = !(tl.pad & MIJ_TILE_STARTS) && (f[-1] & MIJ_PROG_OPEN) != 0; /* the block in front of the tile, of the same scan */
		for (int half = 0; half < 2; ++half) {
			const uint32_t j = (uint32_t)lane + 64u * half;
			if (j >= n)
				continue;
			const bool has = ((half ? S1 : S0) >> lane) & 1u, open = ((half ? E1 : E0) >> lane) & 1u;
			const bool prev_open = j == 0 ? prev_open0 : (j == 64 ? (E0 >> 63) & 1u : ((half ? E1 : E0) >> (lane - 1)) & 1u);
			if (!open || !(has || !prev_open))
				continue; /* closes its band, or lies inside a run another block started */
			/* the first block behind j with an N lane */
			uint32_t jn = n;
			const uint64_t above = lane == 63 ? 0ull : ~((2ull << lane) - 1ull);
			if (!half) {
				if (S0 & above)
					jn = (uint32_t)__ffsll((long long)(S0 & above)) - 1u;
				else if (S1)
					jn = 64u + (uint32_t)__ffsll((long long)S1) - 1u;
			} else if (S1 & above) {
				jn = 64u + (uint32_t)__ffsll((long long)(S1 & above)) - 1u;
			}
			const bool open_end = jn >= n; /* the run leaves the tile */
			if (open_end)
				jn = n;
			uint32_t len = jn - j + (open_end ? after.len : 0u);
			const uint32_t bits = L->ptb[jn - 1] - L->ptb[j] + (half ? tb1 : tb0) + (open_end ? after.bits : 0u);
			if (len >= MIJ_PROG_MAX_RUN || bits > MIJ_PROG_MAX_PENDING) {
				if (p_flag)
					p_flag[tl.slot] = 1u;
				len = len > MIJ_PROG_MAX_RUN ? MIJ_PROG_MAX_RUN : len; /* the slot is refused; the symbol stays in range */
			}
			L->role[j] = len;
		}
	}
	__syncthreads();
}

/* What a block of an AC scan writes.  COUNT: its symbols into hist[2 * 256 ..] (the scan's AC table), nothing placed; otherwise
 * put(position in the block, code, length) per piece, codes from T->code[2].  run: the EOB run this block writes behind its body, 0 for
 * none; fill: the scan's last block.  Returns the block's bits (0 when counting).  Every lane of the wave calls it. */
template <bool COUNT, typename Put>
__device__ __forceinline__ uint32_t prog_ac_block(const EmitTables *__restrict__ T, uint32_t *hist, ProgScanDef sc, int v, int lane, uint32_t run, bool fill,
																  Put put)
{
	const bool inband = lane >= (int)sc.ss && lane <= (int)sc.se;
	const uint32_t a = inband ? (uint32_t)(v < 0 ? -v : v) >> sc.al : 0u;
	const bool isN = sc.ah ? a == 1u : a != 0u, isC = sc.ah && a > 1u;
	const uint64_t below = (1ull << lane) - 1ull;
	const uint64_t Nm = __ballot(isN), Cm = __ballot(isC), Zm = __ballot(inband && a == 0u);
	const int eob = Nm ? prog_msb(Nm) : -1; /* the last N lane: the block's last event */
	int zrl = 0, zr = 0;
	if ((isN || isC) && lane <= eob) {
		/* zeros since the last N lane below; a C lane in between has taken its sixteens already */
		const uint64_t nb = Nm & below;
		const uint64_t since = nb ? ~((2ull << prog_msb(nb)) - 1ull) : ~0ull;
		const int z = __popcll(Zm & below & since);
		const uint64_t pb = Cm & below & since;
		const int zp = pb ? __popcll(Zm & since & ((1ull << prog_msb(pb)) - 1ull)) : 0;
		zrl = (z >> 4) - (zp >> 4);
		zr = z & 15;
	}
	const int n = isN ? 32 - __clz((int)a) : 0;
	const int sym = (zr << 4) + n;
	const int nb_run = run ? 31 - __clz((int)run) : 0;
	if (COUNT) {
		uint32_t *h = hist + 2 * 256;
		if (zrl)
			atomicAdd(&h[0xF0], (uint32_t)zrl);
		if (isN)
			atomicAdd(&h[sym & 255], 1u);
		if (lane == 0 && run)
			atomicAdd(&h[(nb_run << 4) & 255], 1u);
		return 0u;
	}
	const bool ev = zrl > 0 || isN;
	const uint64_t Em = __ballot(ev);
	const uint32_t zl = T->len[2][0xF0], zc = T->code[2][0xF0];
	const uint32_t sl = isN ? (uint32_t)T->len[2][sym & 255] + (uint32_t)n : 0u;
	const uint32_t mine = (uint32_t)zrl * zl + sl;
	const uint32_t incl = wave_incl_scan(mine, lane);
	const uint32_t sym_total = __shfl(incl, 63, 64);
	/* the correction bits in front of this lane's first piece: those of C lanes below the event before this one */
	const uint64_t eb = Em & below;
	const uint64_t below_pe = eb ? (1ull << prog_msb(eb)) - 1ull : 0ull;
	const uint32_t pos = incl - mine + (uint32_t)__popcll(Cm & below_pe);
	const uint32_t pend = (uint32_t)__popcll(Cm & below & ~below_pe); /* the bits this event releases */
	const uint32_t first_len = zrl > 0 ? zl : sl;
	const uint64_t Tm = eob >= 0 ? Cm & ~((2ull << eob) - 1ull) : Cm; /* the tail: C lanes behind the last event (2 << 63 is 0: none) */
	const uint32_t n_tail = (uint32_t)__popcll(Tm);
	const uint32_t body = sym_total + (uint32_t)__popcll(Cm) - n_tail;
	const uint32_t run_len = run ? (uint32_t)T->len[2][(nb_run << 4) & 255] + (uint32_t)nb_run : 0u;
	/* a C lane's bit stands behind the first piece of the next event */
	const uint64_t ea = lane == 63 ? 0ull : Em & ~((2ull << lane) - 1ull);
	const int ne = ea ? __ffsll((long long)ea) - 1 : lane;
	const uint32_t ne_pos = __shfl(pos, ne, 64), ne_first = __shfl(first_len, ne, 64);
	if (ev) {
		uint32_t p = pos;
		if (zrl > 0) {
			put(p, zc, (int)zl);
			p += zl + pend;
			for (int z = 1; z < zrl; ++z, p += zl)
				put(p, zc, (int)zl);
		}
		if (isN)
			put(p, ((uint32_t)T->code[2][sym & 255] << n) | ((v < 0 ? ~a : a) & ((1u << n) - 1u)), (int)sl);
	}
	if (isC) {
		if (ea) {
			const uint64_t ebe = Em & (below | 1ull << lane); /* the event this lane's bit waits behind: the last one up to the lane */
			const uint64_t from = ebe ? ~((1ull << prog_msb(ebe)) - 1ull) : ~0ull;
			put(ne_pos + ne_first + (uint32_t)__popcll(Cm & below & from), a & 1u, 1);
		} else {
			put(body + run_len + (uint32_t)__popcll(Tm & below), a & 1u, 1);
		}
	}
	if (lane == 0) {
		if (run)
			put(body, ((uint32_t)T->code[2][(nb_run << 4) & 255] << nb_run) | (run & ((1u << nb_run) - 1u)), (int)run_len);
		if (fill)
			put(body + run_len + n_tail, 0x7Fu, 7);
	}
	return body + run_len + n_tail + (fill ? 7u : 0u);
}

/* What a unit of a DC scan writes: lane 0's symbol (first scan) or bit (refinement), and the fill */
template <bool COUNT, typename Put>
__device__ __forceinline__ uint32_t prog_dc_unit(const EmitTables *__restrict__ T, uint32_t *hist, ProgScanDef sc, UnitIn in, bool luma, int lane, bool fill,
																 Put put)
{
	uint32_t len = 0;
	if (lane == 0) {
		if (sc.ah) {
			if (!COUNT)
				put(0u, (uint32_t)(in.v >> sc.al) & 1u, 1);
			len = 1;
		} else {
			const int diff = (in.v >> sc.al) - (in.pred >> sc.al); /* arithmetic shifts; a scan's first units predict from 0 */
			uint32_t bits = 0;
			const int n = diff ? emit_mag(diff, bits) : 0;
			const int t = luma ? 0 : 1;
			if (COUNT) {
				atomicAdd(&hist[t * 256 + n], 1u);
			} else {
				len = (uint32_t)T->len[t][n] + (uint32_t)n;
				put(0u, ((uint32_t)T->code[t][n] << n) | bits, (int)len);
			}
		}
		if (fill && !COUNT) {
			put(len, 0x7Fu, 7);
			len += 7;
		}
	}
	return COUNT ? 0u : __shfl(len, 0, 64);
}

/* f(j, bits of block j) for the blocks j = wave, wave + 4, ... of a progressive tile, each written through put(j, position, code, length);
 * the next block's load in flight.  Behind prog_tile_setup. */
template <bool COUNT, typename Put, typename F>
__device__ __forceinline__ void prog_blocks(const EmitTables *__restrict__ T, uint32_t *hist, const EmitSlot &s, const EmitTile &tl, ProgScanDef sc,
														  const int16_t *__restrict__ du, const ProgLds *L, Put put, F f)
{
	const int lane = threadIdx.x & 63;
	const uint32_t n = emit_tile_units(tl);
	const bool fills = (tl.pad & MIJ_TILE_FILLS) != 0;
	uint32_t j = threadIdx.x >> 6;
	if (j >= n)
		return;
	if (sc.ss == 0) {
		UnitIn in = emit_load(s, tl, du, tl.first + j, lane);
		for (; j < n; j += 4) {
			UnitIn next = in;
			if (j + 4 < n)
				next = emit_load(s, tl, du, tl.first + j + 4, lane);
			const uint32_t u = tl.first + j, p = u % s.dpm;
			f(j, prog_dc_unit<COUNT>(T, hist, sc, in, p < s.ny, lane, fills && j + 1 == n, [&](uint32_t pos, uint32_t code, int len) { put(j, pos, code, len); }));
			in = next;
		}
		return;
	}
	int v = du[(size_t)L->uidx[j] * 64 + lane];
	for (; j < n; j += 4) {
		int next = v;
		if (j + 4 < n)
			next = du[(size_t)L->uidx[j + 4] * 64 + lane];
		f(j, prog_ac_block<COUNT>(T, hist, sc, v, lane, L->role[j], fills && j + 1 == n, [&](uint32_t pos, uint32_t code, int len) { put(j, pos, code, len); }));
		v = next;
	}
}

/* emit_pack_tile for a progressive tile */
__device__ void prog_pack_tile(const EmitTables *__restrict__ T, const EmitSlot &s, const EmitTile &tl, ProgScanDef sc, const int16_t *__restrict__ du,
										 uint32_t h, uint32_t nwords, uint32_t *buf, uint32_t *uoff, const ProgLds *L)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t n = emit_tile_units(tl);
	for (uint32_t i = threadIdx.x; i < nwords; i += blockDim.x)
		buf[i] = 0;
	prog_blocks<false>(T, nullptr, s, tl, sc, du, L, [](uint32_t, uint32_t, uint32_t, int) {}, [&](uint32_t j, uint32_t bits) {
		if (lane == 0)
			uoff[j] = bits;
	});
	__syncthreads();
	if (wave == 0) { /* exclusive scan of the block lengths, two per lane */
		const uint32_t a = (uint32_t)(2 * lane) < n ? uoff[2 * lane] : 0u, b = (uint32_t)(2 * lane + 1) < n ? uoff[2 * lane + 1] : 0u;
		const uint32_t incl = wave_incl_scan(a + b, lane);
		if ((uint32_t)(2 * lane) < n)
			uoff[2 * lane] = incl - a - b;
		if ((uint32_t)(2 * lane + 1) < n)
			uoff[2 * lane + 1] = incl - b;
	}
	__syncthreads();
	prog_blocks<false>(T, nullptr, s, tl, sc, du, L, [&](uint32_t j, uint32_t pos, uint32_t code, int len) { lds_put(buf, h + uoff[j] + pos, code, len); },
							 [](uint32_t, uint32_t) {});
	__syncthreads();
}

/* per progressive tile of an AC scan: a byte per block -- MIJ_PROG_HAS, MIJ_PROG_OPEN, its tail bits (at most 62) -- and the tile's summary */
__global__ __launch_bounds__(256) void k_prog_flags(const EmitSlot *__restrict__ slots, const EmitTile *__restrict__ tiles, const uint32_t *__restrict__ ptile,
																		 const ProgSlot *__restrict__ pslots, const uint8_t *__restrict__ du_base, uint8_t *__restrict__ fl,
																		 ProgTileSum *__restrict__ t_sum)
{
	__shared__ ProgLds L;
	const uint32_t g = ptile[blockIdx.x];
	const EmitTile tl = tiles[g];
	const EmitSlot s = slots[tl.slot];
	const ProgSlot &ps = pslots[s.prog - 1u];
	const uint32_t scan = prog_tile_scan(tl), n = emit_tile_units(tl);
	const ProgScanDef sc = k_prog_script[ps.grey][scan];
	const int lane = threadIdx.x & 63;
	if (sc.ss == 0) {
		if (threadIdx.x == 0) {
			const ProgTileSum z = {n | 1u << 31, 0u, 0u, 0u};
			t_sum[g] = z;
		}
		return;
	}
	prog_tile_setup(ps, s, tl, g, sc, nullptr, nullptr, nullptr, &L);
	const int16_t *du = reinterpret_cast<const int16_t *>(du_base + s.du_off);
	uint8_t *out = fl + ps.flag_off[scan] + tl.first;
	for (uint32_t j = threadIdx.x >> 6; j < n; j += 4) {
		const int v = du[(size_t)L.uidx[j] * 64 + lane];
		const bool inband = lane >= (int)sc.ss && lane <= (int)sc.se;
		const uint32_t a = inband ? (uint32_t)(v < 0 ? -v : v) >> sc.al : 0u;
		const uint64_t Nm = __ballot(sc.ah ? a == 1u : a != 0u), Cm = __ballot(sc.ah && a > 1u);
		const uint64_t Tm = Nm ? Cm & ~((2ull << prog_msb(Nm)) - 1ull) : Cm;
		const uint32_t b = (Nm ? MIJ_PROG_HAS : 0u) | (((Nm >> sc.se) & 1u) ? 0u : MIJ_PROG_OPEN) | (uint32_t)__popcll(Tm);
		if (lane == 0) {
			out[j] = (uint8_t)b;
			L.fl[j] = (uint8_t)b;
		}
	}
	__syncthreads();
	if (threadIdx.x < 64) {
		const uint32_t a = L.fl[lane], b = L.fl[lane + 64];
		const uint64_t S0 = __ballot((a & MIJ_PROG_HAS) != 0), S1 = __ballot((b & MIJ_PROG_HAS) != 0);
		const uint32_t P0 = wave_incl_scan(a & 63u, lane), P1 = __shfl(P0, 63, 64) + wave_incl_scan(b & 63u, lane);
		const uint32_t lead = S0 ? (uint32_t)__ffsll((long long)S0) - 1u : (S1 ? 64u + (uint32_t)__ffsll((long long)S1) - 1u : n);
		/* the inclusive sum at block lead - 1, and at the last block (blocks behind n hold 0) */
		const uint32_t at = lead ? lead - 1u : 0u;
		const uint32_t lead_bits = lead ? (at < 64u ? __shfl(P0, (int)at, 64) : __shfl(P1, (int)(at - 64u), 64)) : 0u;
		const uint32_t sum = __shfl(P1, 63, 64);
		if (lane == 0) {
			const ProgTileSum z = {n | ((S0 | S1) ? 1u << 31 : 0u), lead, lead_bits, sum};
			t_sum[g] = z;
		}
	}
}

/* one wave per progressive slot: for every tile, the empty blocks that follow it in its scan and their tail bits -- a segmented scan over the
 * tile summaries in reverse.  An element is (stops, blocks, bits): a tile with an N lane stops the count at its leading empty blocks, a scan's
 * last tile stops it at all of its blocks; (x then y) = x when x stops, else (y's stop, sums).  Lane l of a chunk holds the l-th tile from the
 * end, so what follows a tile is what lane l - 1 has gathered. */
__global__ __launch_bounds__(256) void k_prog_runs(const EmitSlot *__restrict__ slots, const EmitTile *__restrict__ tiles, const ProgSlot *__restrict__ pslots,
																		uint32_t n_prog, const ProgTileSum *__restrict__ t_sum, ProgAfter *__restrict__ t_after)
{
	const int lane = threadIdx.x & 63;
	const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (i >= n_prog)
		return;
	const EmitSlot s = slots[pslots[i].slot];
	uint32_t c_stop = 1, c_len = 0, c_bits = 0; /* what follows the tiles of the chunk */
	for (uint32_t r0 = 0; r0 < s.n_tiles; r0 += 64) {
		const uint32_t r = r0 + (uint32_t)lane;
		const bool live = r < s.n_tiles;
		const uint32_t g = s.first_tile + (live ? s.n_tiles - 1u - r : 0u);
		uint32_t stop = 1, len = 0, bits = 0;
		bool last = true;
		if (live) {
			const ProgTileSum z = t_sum[g];
			const bool has = (z.n_has >> 31) != 0;
			last = (tiles[g].pad & MIJ_TILE_FILLS) != 0;
			stop = has || last;
			len = has ? z.lead : z.n_has & 0x7FFFFFFFu;
			bits = has ? z.lead_bits : z.sum_bits;
		}
		for (int o = 1; o < 64; o <<= 1) {
			const uint32_t ys = __shfl_up(stop, o, 64), yl = __shfl_up(len, o, 64), yb = __shfl_up(bits, o, 64);
			if (lane >= o && !stop) {
				stop = ys;
				len += yl;
				bits += yb;
			}
		}
		if (!stop) { /* open to the end of the chunk: what follows the chunk continues it */
			stop = c_stop;
			len += c_len;
			bits += c_bits;
		}
		const uint32_t pl = __shfl_up(len, 1, 64), pb = __shfl_up(bits, 1, 64);
		if (live) {
			ProgAfter a = {lane ? pl : c_len, lane ? pb : c_bits};
			if (last)
				a.len = a.bits = 0;
			t_after[g] = a;
		}
		c_stop = __shfl(stop, 63, 64);
		c_len = __shfl(len, 63, 64);
		c_bits = __shfl(bits, 63, 64);
	}
}

/* per progressive tile: the symbols of its blocks, the EOBn of the runs they start included, added to the scan's counts
 * freq[(prog - 1) * MIJ_PROG_SCANS + scan][4][256]: DC tables in [0] and [1], the AC table in [2] */
__global__ __launch_bounds__(256) void k_prog_hist(const EmitSlot *__restrict__ slots, const EmitTile *__restrict__ tiles, const uint32_t *__restrict__ ptile,
																		const ProgSlot *__restrict__ pslots, const uint8_t *__restrict__ du_base,
																		const uint8_t *__restrict__ fl, const ProgAfter *__restrict__ t_after, uint32_t *__restrict__ freq,
																		uint32_t *__restrict__ p_flag)
{
	__shared__ ProgLds L;
	__shared__ uint32_t hist[3 * 256];
	const uint32_t g = ptile[blockIdx.x];
	const EmitTile tl = tiles[g];
	const EmitSlot s = slots[tl.slot];
	const ProgSlot &ps = pslots[s.prog - 1u];
	const uint32_t scan = prog_tile_scan(tl);
	const ProgScanDef sc = k_prog_script[ps.grey][scan];
	if (sc.ss == 0 && sc.ah)
		return; /* DC refinement has no symbols */
	for (uint32_t i = threadIdx.x; i < 3 * 256; i += blockDim.x)
		hist[i] = 0;
	prog_tile_setup(ps, s, tl, g, sc, fl, t_after, p_flag, &L);
	prog_blocks<true>(nullptr, hist, s, tl, sc, reinterpret_cast<const int16_t *>(du_base + s.du_off), &L, [](uint32_t, uint32_t, uint32_t, int) {},
							[](uint32_t, uint32_t) {});
	__syncthreads();
	uint32_t *out = freq + (size_t)((s.prog - 1u) * MIJ_PROG_SCANS + scan) * (4 * 256);
	for (uint32_t i = threadIdx.x; i < 3 * 256; i += blockDim.x)
		if (hist[i])
			atomicAdd(&out[i], hist[i]);
}
