/*
 * mij_emit_kernels.h -- the JPEG writer's Huffman stage on the GPU (mij_enc_stream_reserve, include/mij.h), and the gather kernel
 * of encoder slots whose pixels are device memory (mij_enc_add_device).  Included by mij_runtime.hip.
 *
 * Emission reproduces mjw_emit (csrc/jpeg_write_host.c; codec/jpeg_write.c:120-169, :245-268, :358-363) byte for byte.  A slot's
 * data units are cut into tiles of MIJ_EMIT_TILE consecutive units, one workgroup each, one wavefront per unit: lane k holds zigzag
 * coefficient k, a ballot gives the non-zero mask, and each lane owns the bits of its own symbol -- lane 0 the DC difference, a
 * non-zero lane k its ZRLs (0xF0 per 16 zeros) and its run/size symbol, lane 63 also the EOB when coefficient 63 is zero and, in a
 * slot's last unit, the 7 one-bits of fill.  A wave prefix sum of the lane lengths places every symbol.  Six launches, each over
 * a work list (so their number does not grow with the slot count), with kernel boundaries as the only hand-offs:
 *   k_emit_len     per tile: the sum of its units' bit lengths
 *   k_emit_scan    one wave per slot: each tile's bit offset in its slot, the slot's bit total
 *   k_emit_count   per tile: its bits packed in LDS; the 0xFF bytes among the bytes whose 8 bits all lie in the tile, and the
 *                  tile's head and tail fragments (its bits before its first and after its last byte boundary)
 *   k_emit_stuff   one wave per slot: each tile's stuffed size (a byte shared by two tiles -- the previous tail and this head --
 *                  belongs to the tile holding its last bit) scanned into its output offset; the slot's entropy bytes
 *   k_emit_place   one workgroup: slot lengths scanned into arena offsets in slot order; which slots fit
 *   k_emit_write   per tile of a slot that fits: its bits packed again, stuffed and stored at their final offset; the slot's
 *                  first tile stores the headers, its last tile the EOI
 * Bits left below a byte after the fill are dropped (they are the last tile's tail).  Nothing but the streams of fitting slots is
 * written to the arena, and the data units are only read.
 *
 * Restart intervals (mij_enc_set_restart; the contract is include/mij_host.h, RESTART INTERVALS): the same launches.  The tile list of a slot
 * with an interval is cut so that no tile straddles an interval end (EmitTile.pad: unit count, "ends interval k"); a tile is then either
 * MIJ_EMIT_TILE units long or ends an interval with the 7 fill bits, so it never holds less than a byte.  emit_load predicts an interval's
 * first units from 0 and the fill's owner is every interval's last unit (both read from the tile's flags, no division by the interval); k_emit_scan's offsets restart at each interval (a segmented scan),
 * which makes an interval's first tile start at a byte boundary and its last tile's tail the dropped remainder; k_emit_stuff adds the two
 * marker bytes behind an interval's last tile and k_emit_write stores them there.  k_emit_build puts the DRI segment in front of SOS.
 * A slot without an interval has one tile per MIJ_EMIT_TILE units and no flag, and every kernel computes for it what it computed before.
 *
 * Optimised Huffman tables (mij_enc_set_optimize; the contract is mjw_emit_optimized's, include/mij_host.h): two more launches in
 * front of the six, over the optimised slots only, and none when there is no such slot:
 *   k_emit_hist    per tile of an optimised slot: the symbols its lanes own, counted in an LDS histogram and added to the slot's
 *                  uint32 [4][256] counts
 *   k_emit_build   one workgroup per optimised slot, one wavefront per table: ITU-T T.81 K.2 on the counts (libjpeg's tie-breaking),
 *                  the slot's EmitTables entry, its DHT segment and header length; a slot with a code above 32 bits before the
 *                  shortening keeps table 0 (the plain tables) and the plain header
 * The tile kernels read the tables their EmitTile.tab names -- in the tile's own entry, so that the copy of the tables into LDS waits
 * for that entry alone and not for the slot's as well -- and the header length EmitSlot.hlen.
 *
 * Progressive output (mij_enc_set_progressive; the contract is include/mij_host.h, PROGRESSIVE STREAMS): mij_progressive_kernels.h.  A scan is
 * a segment as a restart interval is, so the six launches write such a slot too: the tile kernels branch once per tile on EmitSlot.prog
 * (prog_tile_setup, prog_blocks, prog_pack_tile in place of emit_units / emit_pack_tile), k_emit_scan restarts the offsets behind every scan,
 * k_emit_stuff adds the next scan's header where it adds a marker, and -- a progressive tile can hold less than a byte, even nothing -- also
 * carries each tile's partial byte across such tiles (ProgArgs.ctail), which k_emit_write completes the next byte from.  Four launches in
 * front (k_prog_flags, k_prog_runs, k_prog_hist, k_prog_build), none without a progressive slot.  A slot without the request takes the
 * branches it took before.
 */
#pragma once

#define MIJ_EMIT_TILE 128
#define MIJ_EMIT_HDR 629 /* MJW_LJ_HEADER_BYTES: the stride of the header list, and the longest header */
/* most bits a unit within the writer's ranges takes: chroma DC 11 + 11, 63 AC symbols of 16 + 10, the 7 fill bits */
#define MIJ_EMIT_MAX_DU_BITS (22 + 63 * 26 + 7)
#define MIJ_EMIT_LDS_WORDS ((MIJ_EMIT_TILE * MIJ_EMIT_MAX_DU_BITS + 7 + 31) / 32 + 1)

struct EmitTables {
	uint16_t code[4][256]; /* luma DC, chroma DC, luma AC, chroma AC */
	uint8_t len[4][256];
};

struct EmitSlot {
	uint64_t du_off; /* bytes into the data-unit arena */
	uint32_t n_du, dpm; /* units; units per MCU: 6 (4:2:0), 3 (4:4:4) and, for coefficient slots (mij_enc_add_coef), 4 (4:2:2, 4:4:0) or 1 (grey) */
	uint32_t first_tile, n_tiles;
	uint32_t hdr, tab; /* header of the slot: hdrs + hdr * MIJ_EMIT_HDR; tab > 0: optimised, its tables are entry tab, its counts tab - 1 */
	uint32_t hlen, ny; /* the header's length: what the upload wrote, or what k_emit_build wrote; luma units per MCU (1, 2 or 4): unit p of an MCU is luma when p < ny */
	uint32_t ri, prog; /* the restart interval in MCUs (mij_enc_set_restart), 0: none; prog > 0: a progressive slot (mij_enc_set_progressive), ProgSlot prog - 1 */
	uint32_t lj, pad;  /* lj: the header is in libjpeg's framing (mij_enc_set_arith; mij_host.h, LIBJPEG ENCODING): a DQT and a DHT segment per table */
};

struct EmitTile {
	uint32_t slot, first; /* the tile's first unit in its slot */
	uint32_t tab, pad;    /* the tables the tile kernels use: entry 0 (plain), or what k_emit_build wrote; pad: emit_tile_pad */
};
/* EmitTile.pad: the tile's unit count (1..MIJ_EMIT_TILE; no tile straddles an interval end) in bits 0-8; MIJ_TILE_ENDS when the tile's last
 * unit ends a restart interval that a marker follows (not the slot's last), with that interval's number mod 8 in bits 10-12;
 * MIJ_TILE_STARTS when the tile's first MCU is the first of an interval or of the slot (its units predict from 0); MIJ_TILE_FILLS when its last
 * unit is the last of an interval or of the slot (the 7 fill bits follow it).  A slot without an interval has STARTS on its first tile, FILLS on
 * its last and never ENDS.  The kernels take what depends on the interval from these flags: no division by it anywhere. */
/* A progressive slot's tiles (mij_progressive_kernels.h) also carry their scan in bits 16-19; a scan is a segment as an interval is: ENDS on the
 * last tile of a scan that another follows, whose header then stands where the marker would. */
#define MIJ_TILE_ENDS 0x200u
#define MIJ_TILE_STARTS 0x2000u
#define MIJ_TILE_FILLS 0x4000u
__host__ __device__ __forceinline__ uint32_t emit_tile_pad(uint32_t n, bool starts, bool fills, bool ends, uint32_t k)
{
	return n | (starts ? MIJ_TILE_STARTS : 0u) | (fills ? MIJ_TILE_FILLS : 0u) | (ends ? MIJ_TILE_ENDS | (k & 7u) << 10 : 0u);
}
__device__ __forceinline__ uint32_t emit_tile_units(const EmitTile &tl) { return tl.pad & 0x1FFu; }

struct EmitResult {
	uint64_t off, len; /* off = ~0 for a slot that does not fit; entry n: {bytes used, slots that fit} */
};

/* the magnitude category of v != 0 and the bits that follow it (codec/jpeg_write.c:76-86) */
__device__ __forceinline__ int emit_mag(int v, uint32_t &bits)
{
	const uint32_t a = (uint32_t)(v < 0 ? -v : v);
	const int n = 32 - __clz((int)a);
	bits = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u);
	return n;
}

/* What lane `lane` emits for unit u of a slot: zrl ZRL codes, then sym, then extra (EOB and / or fill). */
struct LaneBits {
	uint32_t sym, extra, zrl_code;
	int sym_len, extra_len, zrl_len, zrl;
	__device__ int total() const { return zrl * zrl_len + sym_len + extra_len; }
};
struct UnitIn {
	int v, pred; /* this lane's coefficient; the DC predictor (lane 0) */
};
/* the loads of unit u of tile tl (issued a unit ahead of its use: emit_units) */
__device__ __forceinline__ UnitIn emit_load(const EmitSlot &s, const EmitTile &tl, const int16_t *__restrict__ du, uint32_t u, int lane)
{
	const uint32_t m = u / s.dpm, p = u - m * s.dpm;
	/* the unit whose DC predicts this one's, the previous unit of the component in MCU order: u - 1 inside an MCU's luma run, the last luma unit
	 * of the MCU before for its first, the same unit of the MCU before for chroma */
	const long back = p < s.ny ? (long)(s.dpm - s.ny + 1u) : (long)s.dpm;
	/* an interval's first MCU (the slot's first without an interval) has no MCU before it: the first MCU of a tile that starts one */
	const bool first_mcu = (tl.pad & MIJ_TILE_STARTS) && u - tl.first < s.dpm;
	const long prev = p > 0 && p < s.ny ? (long)u - 1 : (!first_mcu ? (long)u - back : -1);
	UnitIn in;
	in.v = du[(size_t)u * 64 + lane];
	in.pred = lane == 0 && prev >= 0 ? (int)du[(size_t)prev * 64] : 0;
	return in;
}
/* Which lane owns which symbol of unit u, said once for the emission kernels and for the histogram: own.dc(category, bits) in lane
 * 0, own.ac(ZRLs, run/size symbol, size, bits) in a lane k > 0 whose coefficient is non-zero (the ZRLs, 0xF0 per 16 zeros of its run,
 * come before the symbol), own.eob() in lane 63 when coefficient 63 is zero; own.begin(luma) first.  Every lane of the wave must call
 * it for the same unit (ballot). */
template <typename Own>
__device__ __forceinline__ void emit_owner(const EmitSlot &s, UnitIn in, uint32_t u, int lane, Own &own)
{
	const uint32_t m = u / s.dpm, p = u - m * s.dpm;
	const bool luma = p < s.ny;
	const int v = in.v;
	const uint64_t nz = __ballot(v != 0) & ~1ull;
	own.begin(luma);
	if (lane == 0) {
		const int diff = v - in.pred;
		if (diff == 0) {
			own.dc(0, 0u);
		} else {
			uint32_t bits;
			const int n = emit_mag(diff, bits);
			own.dc(n, bits);
		}
	} else if (v != 0) {
		const uint64_t below = nz & ((1ull << lane) - 1ull);
		const int last = below ? 63 - __clzll((long long)below) : 0;
		const int run = lane - last - 1;
		uint32_t bits;
		const int n = emit_mag(v, bits), sym = ((run & 15) << 4) + n;
		own.ac(run >> 4, sym & 255, n, bits);
	}
	if (lane == 63 && v == 0)
		own.eob();
}

/* the owner that looks the symbols up in T */
struct LaneCoder {
	const EmitTables *__restrict__ T;
	LaneBits &L;
	int dcT, acT;
	__device__ __forceinline__ void begin(bool luma)
	{
		dcT = luma ? 0 : 1;
		acT = luma ? 2 : 3;
		L.sym = L.extra = L.zrl_code = 0;
		L.sym_len = L.extra_len = L.zrl_len = L.zrl = 0;
	}
	__device__ __forceinline__ void dc(int n, uint32_t bits)
	{
		L.sym = ((uint32_t)T->code[dcT][n] << n) | bits;
		L.sym_len = T->len[dcT][n] + n;
	}
	__device__ __forceinline__ void ac(int zrl, int sym, int n, uint32_t bits)
	{
		L.zrl = zrl;
		L.zrl_code = T->code[acT][0xF0];
		L.zrl_len = T->len[acT][0xF0];
		L.sym = ((uint32_t)T->code[acT][sym] << n) | bits;
		L.sym_len = T->len[acT][sym] + n;
	}
	__device__ __forceinline__ void eob()
	{
		L.extra = T->code[acT][0];
		L.extra_len = T->len[acT][0];
	}
};
__device__ __forceinline__ void emit_lane(const EmitTables *__restrict__ T, const EmitSlot &s, const EmitTile &tl, UnitIn in, uint32_t u, int lane, LaneBits &L)
{
	LaneCoder c = {T, L, 0, 0};
	emit_owner(s, in, u, lane, c);
	/* the slot's last unit, and the last unit of a restart interval: fill to a byte boundary with ones */
	if (lane == 63 && (tl.pad & MIJ_TILE_FILLS) && u + 1 == tl.first + emit_tile_units(tl)) {
		L.extra = (L.extra << 7) | 0x7Fu;
		L.extra_len += 7;
	}
}

/* f(j, u, UnitIn) for the units j = wave, wave + 4, ... < n of tile tl (u = tl.first + j), the next unit's loads in flight */
template <typename F>
__device__ __forceinline__ void emit_unit_loop(const EmitSlot &s, const EmitTile &tl, const int16_t *__restrict__ du, F f)
{
	const int lane = threadIdx.x & 63;
	const uint32_t first = tl.first, n = emit_tile_units(tl);
	uint32_t j = threadIdx.x >> 6;
	if (j >= n)
		return;
	UnitIn in = emit_load(s, tl, du, first + j, lane);
	for (; j < n; j += 4) {
		UnitIn next = in;
		if (j + 4 < n)
			next = emit_load(s, tl, du, first + j + 4, lane);
		f(j, first + j, in);
		in = next;
	}
}
/* f(j, LaneBits) for those units, their symbols looked up in T */
template <typename F>
__device__ __forceinline__ void emit_units(const EmitTables *__restrict__ T, const EmitSlot &s, const EmitTile &tl, const int16_t *__restrict__ du, F f)
{
	const int lane = threadIdx.x & 63;
	emit_unit_loop(s, tl, du, [&](uint32_t j, uint32_t u, UnitIn in) {
		LaneBits L;
		emit_lane(T, s, tl, in, u, lane, L);
		f(j, L);
	});
}

/* the code tables into LDS (every workgroup of the tile kernels; blockDim.x = 256) */
__device__ __forceinline__ void emit_tables_to_lds(const EmitTables *__restrict__ g, EmitTables *t)
{
	const uint32_t *src = reinterpret_cast<const uint32_t *>(g);
	uint32_t *dst = reinterpret_cast<uint32_t *>(t);
	for (uint32_t i = threadIdx.x; i < sizeof(EmitTables) / 4; i += blockDim.x)
		dst[i] = src[i];
	__syncthreads();
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
	for (int o = 32; o > 0; o >>= 1)
		v += __shfl_xor(v, o, 64);
	return v;
}
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane)
{
	for (int o = 1; o < 64; o <<= 1) {
		const uint32_t t = __shfl_up(v, o, 64);
		if (lane >= o)
			v += t;
	}
	return v;
}

/* code (right-aligned, len <= 32 bits) at bit pos of an MSB-first LDS bit buffer; lanes own disjoint bit ranges */
__device__ __forceinline__ void lds_put(uint32_t *buf, uint32_t pos, uint32_t code, int len)
{
	if (len <= 0)
		return;
	const uint32_t w = pos >> 5, o = pos & 31u;
	const uint64_t v = (uint64_t)code << (64 - len - (int)o);
	atomicOr(&buf[w], (uint32_t)(v >> 32));
	if (o + (uint32_t)len > 32u)
		atomicOr(&buf[w + 1], (uint32_t)v);
}
__device__ __forceinline__ uint32_t lds_byte(const uint32_t *buf, uint32_t j) { return (buf[j >> 2] >> (24 - 8 * (j & 3u))) & 0xFFu; }

#include "mij_progressive_kernels.h"

/* what the tile kernels need of a launch's progressive slots: all NULL without one */
struct ProgArgs {
	const ProgSlot *slots;
	const uint8_t *fl;      /* k_prog_flags' block bytes */
	const ProgAfter *after; /* k_prog_runs' per-tile results */
	const uint8_t *hdr;     /* scan headers behind the first: entry (prog - 1) * MIJ_PROG_SCANS + scan, MIJ_PROG_HDR bytes each */
	const uint32_t *hlen;   /* their lengths */
	uint32_t *ctail;        /* per tile: the partial byte behind it, bits of earlier tiles included (k_emit_stuff) */
};

/* Packs tile tl's bits into buf from bit h on (buf zeroed here; nwords of it are used).  uoff: MIJ_EMIT_TILE + 1 words of LDS. */
__device__ void emit_pack_tile(const EmitTables *__restrict__ T, const EmitSlot &s, const EmitTile &tl, const int16_t *__restrict__ du, uint32_t h,
										 uint32_t nwords, uint32_t *buf, uint32_t *uoff)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t n = emit_tile_units(tl);
	for (uint32_t i = threadIdx.x; i < nwords; i += blockDim.x)
		buf[i] = 0;
	emit_units(T, s, tl, du, [&](uint32_t j, const LaneBits &L) {
		const uint32_t t = wave_sum((uint32_t)L.total());
		if (lane == 0)
			uoff[j] = t;
	});
	__syncthreads();
	if (wave == 0) { /* exclusive scan of the unit lengths, two per lane */
		const uint32_t a = (uint32_t)(2 * lane) < n ? uoff[2 * lane] : 0u, b = (uint32_t)(2 * lane + 1) < n ? uoff[2 * lane + 1] : 0u;
		const uint32_t incl = wave_incl_scan(a + b, lane);
		if ((uint32_t)(2 * lane) < n)
			uoff[2 * lane] = incl - a - b;
		if ((uint32_t)(2 * lane + 1) < n)
			uoff[2 * lane + 1] = incl - b;
	}
	__syncthreads();
	emit_units(T, s, tl, du, [&](uint32_t j, const LaneBits &L) {
		const uint32_t len = (uint32_t)L.total();
		uint32_t pos = h + uoff[j] + wave_incl_scan(len, lane) - len;
		for (int z = 0; z < L.zrl; ++z, pos += (uint32_t)L.zrl_len)
			lds_put(buf, pos, L.zrl_code, L.zrl_len);
		lds_put(buf, pos, L.sym, L.sym_len);
		lds_put(buf, pos + (uint32_t)L.sym_len, L.extra, L.extra_len);
	});
	__syncthreads();
}

__global__ __launch_bounds__(256) void k_emit_len(const EmitSlot *__restrict__ slots, const EmitTile *__restrict__ tiles,
																  const EmitTables *__restrict__ T, const uint8_t *__restrict__ du_base, uint32_t *__restrict__ t_bits, ProgArgs pa)
{
	__shared__ uint32_t part[4];
	__shared__ EmitTables tab;
	__shared__ ProgLds pl;
	const EmitTile tl = tiles[blockIdx.x];
	const EmitSlot s = slots[tl.slot];
	const int16_t *du = reinterpret_cast<const int16_t *>(du_base + s.du_off);
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	emit_tables_to_lds(T + tl.tab, &tab);
	uint32_t acc = 0;
	if (s.prog) {
		const ProgSlot &ps = pa.slots[s.prog - 1u];
		const ProgScanDef sc = k_prog_script[ps.grey][prog_tile_scan(tl)];
		prog_tile_setup(ps, s, tl, blockIdx.x, sc, pa.fl, pa.after, nullptr, &pl);
		prog_blocks<false>(&tab, nullptr, s, tl, sc, du, &pl, [](uint32_t, uint32_t, uint32_t, int) {}, [&](uint32_t, uint32_t bits) { acc += bits; });
	} else {
		emit_units(&tab, s, tl, du, [&](uint32_t, const LaneBits &L) { acc += wave_sum((uint32_t)L.total()); });
	}
	if (lane == 0)
		part[wave] = acc;
	__syncthreads();
	if (threadIdx.x == 0)
		t_bits[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

__device__ __forceinline__ uint64_t wave_incl_max64(uint64_t v, int lane)
{
	for (int o = 1; o < 64; o <<= 1) {
		const uint64_t t = __shfl_up(v, o, 64);
		if (lane >= o)
			v = t > v ? t : v;
	}
	return v;
}

/* one wave per slot: each tile's bit offset in its restart interval -- in its slot, for a slot without one.  A segmented scan: the bits behind an
 * interval end start at a byte boundary again, so a tile's offset is its offset in the slot less that of the tile its interval began with;
 * offsets only grow, so that one is the largest among the interval starts up to the tile (a running maximum, carried across the chunks in
 * `seg`).  Every lane runs every step. */
__global__ __launch_bounds__(256) void k_emit_scan(const EmitSlot *__restrict__ slots, const EmitTile *__restrict__ tiles, uint32_t n_slots,
																	const uint32_t *__restrict__ t_bits, uint64_t *__restrict__ t_boff)
{
	const int lane = threadIdx.x & 63;
	const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (i >= n_slots)
		return;
	const EmitSlot s = slots[i];
	uint64_t base = 0, seg = 0;
	for (uint32_t t0 = 0; t0 < s.n_tiles; t0 += 64) {
		const uint32_t t = t0 + (uint32_t)lane;
		const uint32_t v = t < s.n_tiles ? t_bits[s.first_tile + t] : 0u;
		const uint32_t incl = wave_incl_scan(v, lane);
		const uint64_t excl = base + incl - v;
		uint64_t from = 0;
		if (s.ri | s.prog) { /* the same in every lane of the wave: a slot without an interval or scans skips the tile flags and the second scan */
			const bool starts = t > 0 && t < s.n_tiles && (tiles[s.first_tile + t - 1].pad & MIJ_TILE_ENDS) != 0;
			from = wave_incl_max64(starts ? excl : seg, lane);
		}
		if (t < s.n_tiles)
			t_boff[s.first_tile + t] = excl - from;
		seg = __shfl(from, 63, 64);
		base += __shfl(incl, 63, 64);
	}
}

/* per tile: the 0xFF bytes among those whose 8 bits all lie in the tile, and the head / tail fragments (t_frag = head | tail << 8) */
__global__ __launch_bounds__(256) void k_emit_count(const EmitSlot *__restrict__ slots, const EmitTile *__restrict__ tiles,
																	 const EmitTables *__restrict__ T, const uint8_t *__restrict__ du_base, const uint32_t *__restrict__ t_bits,
																	 const uint64_t *__restrict__ t_boff, uint32_t *__restrict__ t_ff, uint32_t *__restrict__ t_frag,
																	 const uint32_t *__restrict__ s_flag, const uint32_t *__restrict__ p_flag, ProgArgs pa)
{
	__shared__ uint32_t buf[MIJ_EMIT_LDS_WORDS];
	__shared__ uint32_t uoff[MIJ_EMIT_TILE + 1];
	__shared__ uint32_t part[4];
	__shared__ EmitTables tab;
	__shared__ ProgLds pl;
	const EmitTile tl = tiles[blockIdx.x];
	const EmitSlot s = slots[tl.slot];
	const uint64_t b0 = t_boff[blockIdx.x], b1 = b0 + t_bits[blockIdx.x];
	const uint32_t h = (uint32_t)(b0 & 7u), n_own = (uint32_t)((b1 >> 3) - (b0 >> 3));
	const uint32_t nwords = (uint32_t)((h + (b1 - b0) + 31) / 32);
	/* units outside the writer's ranges: the slot is refused (k_emit_stuff) before anything is packed -- a coefficient slot the conversion
	 * kernel flagged (s_flag, NULL when the launch has no such slot), or a tile longer than the ranges allow */
	/* a progressive slot with a forced flush or without a table (p_flag, NULL without a progressive slot) goes the same way */
	if ((s_flag && s_flag[tl.slot]) || (p_flag && p_flag[tl.slot]) || nwords > MIJ_EMIT_LDS_WORDS - 1) {
		if (threadIdx.x == 0) {
			t_ff[blockIdx.x] = ~0u;
			t_frag[blockIdx.x] = 0;
		}
		return;
	}
	emit_tables_to_lds(T + tl.tab, &tab);
	if (s.prog) {
		const ProgSlot &ps = pa.slots[s.prog - 1u];
		const ProgScanDef sc = k_prog_script[ps.grey][prog_tile_scan(tl)];
		prog_tile_setup(ps, s, tl, blockIdx.x, sc, pa.fl, pa.after, nullptr, &pl);
		prog_pack_tile(&tab, s, tl, sc, reinterpret_cast<const int16_t *>(du_base + s.du_off), h, nwords, buf, uoff, &pl);
	} else {
		emit_pack_tile(&tab, s, tl, reinterpret_cast<const int16_t *>(du_base + s.du_off), h, nwords, buf, uoff);
	}
	uint32_t c = 0;
	for (uint32_t j = (h ? 1u : 0u) + threadIdx.x; j < n_own; j += blockDim.x)
		c += lds_byte(buf, j) == 0xFFu;
	c = wave_sum(c);
	if ((threadIdx.x & 63) == 0)
		part[threadIdx.x >> 6] = c;
	__syncthreads();
	if (threadIdx.x == 0) {
		const uint32_t tb = (uint32_t)(b1 & 7u);
		const uint32_t head = h && n_own ? lds_byte(buf, 0) & ((1u << (8 - h)) - 1u) : 0u;
		const uint32_t tail = tb ? lds_byte(buf, n_own) >> (8 - tb) : 0u;
		t_ff[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
		t_frag[blockIdx.x] = head | tail << 8;
	}
}

/* one wave per slot: each tile's offset in the stuffed entropy-coded segment, and the segment's size (~0: refused) */
__global__ __launch_bounds__(256) void k_emit_stuff(const EmitSlot *__restrict__ slots, const EmitTile *__restrict__ tiles, uint32_t n_slots,
																	 const uint32_t *__restrict__ t_bits,
																	 const uint64_t *__restrict__ t_boff, const uint32_t *__restrict__ t_ff, const uint32_t *__restrict__ t_frag,
																	 uint64_t *__restrict__ t_out, uint64_t *__restrict__ s_ent, ProgArgs pa)
{
	const int lane = threadIdx.x & 63;
	const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (i >= n_slots)
		return;
	const EmitSlot s = slots[i];
	uint64_t base = 0;
	bool bad = false;
	uint32_t c_len = 0, c_val = 0; /* progressive: the partial byte the chunk before leaves */
	for (uint32_t t0 = 0; t0 < s.n_tiles; t0 += 64) {
		const uint32_t t = t0 + (uint32_t)lane, g = s.first_tile + t;
		uint32_t v = 0, prev_tail = 0;
		if (s.prog) {
			/* A progressive tile can hold less than a byte, even nothing (blocks inside an EOB run), so a byte can gather bits of many tiles.
			 * The partial byte behind each tile, as a segmented scan: a tile that completes a byte, or starts a scan, starts afresh with its
			 * own tail; any other appends its few bits to what came before.  Every lane runs every step. */
			uint32_t rs = 1, ln = 0, vl = 0;
			if (t < s.n_tiles && t_ff[g] != ~0u) {
				const uint64_t b0 = t_boff[g], b1 = b0 + t_bits[g];
				rs = (b1 >> 3) != (b0 >> 3) || (tiles[g].pad & MIJ_TILE_STARTS) ? 1u : 0u;
				ln = rs ? (uint32_t)(b1 & 7u) : t_bits[g];
				vl = t_frag[g] >> 8;
			}
			for (int o = 1; o < 64; o <<= 1) {
				const uint32_t xs = __shfl_up(rs, o, 64), xl = __shfl_up(ln, o, 64), xv = __shfl_up(vl, o, 64);
				if (lane >= o && !rs) {
					vl |= xv << ln;
					ln += xl;
					rs = xs;
				}
			}
			if (!rs) {
				vl |= c_val << ln;
				ln += c_len;
			}
			const uint32_t up = __shfl_up(vl, 1, 64);
			prev_tail = lane ? up : c_val;
			c_len = __shfl(ln, 63, 64);
			c_val = __shfl(vl, 63, 64);
			if (t < s.n_tiles)
				pa.ctail[g] = vl & 0xFFu;
		}
		if (t < s.n_tiles) {
			const uint64_t b0 = t_boff[g], b1 = b0 + t_bits[g];
			const uint32_t h = (uint32_t)(b0 & 7u), ff = t_ff[g];
			if (ff == ~0u) {
				bad = true;
			} else {
				v = (uint32_t)((b1 >> 3) - (b0 >> 3)) + ff;
				if (h && t > 0) { /* the byte shared with the previous tile */
					const uint32_t byte = ((s.prog ? prev_tail : t_frag[g - 1] >> 8) << (8 - h)) | (t_frag[g] & 0xFFu);
					v += byte == 0xFFu && (b1 >> 3) != (b0 >> 3);
				}
				/* the two marker bytes behind an interval end are added here, in byte space: they never pass through the stuffing.  The interval's
				 * filled last byte is an ordinary whole byte of its tile and was counted as one (t_ff, or the shared byte above) */
				if (s.ri && (tiles[g].pad & MIJ_TILE_ENDS))
					v += 2u;
				/* behind a scan's last tile: the header of the next scan */
				if (s.prog && (tiles[g].pad & MIJ_TILE_ENDS))
					v += pa.hlen[(s.prog - 1u) * MIJ_PROG_SCANS + prog_tile_scan(tiles[g]) + 1u];
			}
		}
		const uint32_t incl = wave_incl_scan(v, lane);
		if (t < s.n_tiles)
			t_out[g] = base + incl - v;
		base += __shfl(incl, 63, 64);
	}
	bad = __ballot(bad) != 0;
	if (lane == 0)
		s_ent[i] = bad ? ~0ull : base;
}

/* one workgroup of 1024: every slot's length and offset in slot order; res[n_slots] = {bytes used, slots that fit} */
__global__ __launch_bounds__(1024) void k_emit_place(const EmitSlot *__restrict__ slots, uint32_t n_slots, const uint64_t *__restrict__ s_ent, uint64_t cap,
																		  EmitResult *__restrict__ res)
{
	__shared__ uint64_t wsum[16];
	__shared__ unsigned long long used, nfit;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	if (threadIdx.x == 0)
		used = nfit = 0;
	uint64_t carry = 0;
	for (uint32_t i0 = 0; i0 < n_slots; i0 += 1024) {
		const uint32_t i = i0 + threadIdx.x;
		const uint64_t ent = i < n_slots ? s_ent[i] : 0;
		const bool bad = ent == ~0ull;
		const uint64_t len = i < n_slots && !bad ? slots[i].hlen + ent + 2 : 0;
		uint64_t incl = len;
		for (int o = 1; o < 64; o <<= 1) {
			const uint64_t t = __shfl_up(incl, o, 64);
			if (lane >= o)
				incl += t;
		}
		if (lane == 63)
			wsum[wave] = incl;
		__syncthreads();
		uint64_t before = carry;
		for (int w = 0; w < wave; ++w)
			before += wsum[w];
		uint64_t total = carry;
		for (int w = 0; w < 16; ++w)
			total += wsum[w];
		const uint64_t off = before + incl - len;
		if (i < n_slots) {
			/* offsets only grow, so the slots that fit are a prefix of the slot order */
			const bool fits = !bad && off + len <= cap;
			res[i].off = fits ? off : ~0ull;
			res[i].len = len;
			if (fits) {
				atomicMax(&used, (unsigned long long)(off + len));
				atomicAdd(&nfit, 1ull);
			}
		}
		carry = total;
		__syncthreads();
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		res[n_slots].off = used;
		res[n_slots].len = nfit;
	}
}

/* per tile of a slot that fits: the tile's bytes, stuffed, at their final offset; the headers and the EOI */
__global__ __launch_bounds__(256) void k_emit_write(const EmitSlot *__restrict__ slots, const EmitTile *__restrict__ tiles,
																	 const EmitTables *__restrict__ T, const uint8_t *__restrict__ du_base, const uint8_t *__restrict__ hdrs,
																	 const uint32_t *__restrict__ t_bits, const uint64_t *__restrict__ t_boff, const uint32_t *__restrict__ t_frag,
																	 const uint64_t *__restrict__ t_out, const EmitResult *__restrict__ res, uint8_t *__restrict__ arena, ProgArgs pa)
{
	__shared__ uint32_t buf[MIJ_EMIT_LDS_WORDS];
	__shared__ uint32_t uoff[MIJ_EMIT_TILE + 1];
	__shared__ uint32_t part[4];
	__shared__ EmitTables tab;
	__shared__ ProgLds pl;
	const EmitTile tl = tiles[blockIdx.x];
	const EmitResult r = res[tl.slot];
	if (r.off == ~0ull)
		return;
	const EmitSlot s = slots[tl.slot];
	uint8_t *out = arena + r.off;
	if (tl.first == 0 && prog_tile_scan(tl) == 0) /* a progressive slot's later scans start at block 0 again */
		for (uint32_t i = threadIdx.x; i < s.hlen; i += blockDim.x)
			out[i] = hdrs[(size_t)s.hdr * MIJ_EMIT_HDR + i];
	const bool last_tile = s.prog ? (tl.pad & (MIJ_TILE_FILLS | MIJ_TILE_ENDS)) == MIJ_TILE_FILLS : tl.first + emit_tile_units(tl) >= s.n_du;
	if (last_tile && threadIdx.x == 0) {
		out[r.len - 2] = 0xFF;
		out[r.len - 1] = 0xD9;
	}
	const uint64_t b0 = t_boff[blockIdx.x], b1 = b0 + t_bits[blockIdx.x];
	const uint32_t h = (uint32_t)(b0 & 7u), n_own = (uint32_t)((b1 >> 3) - (b0 >> 3));
	const uint32_t nwords = (uint32_t)((h + (b1 - b0) + 31) / 32);
	emit_tables_to_lds(T + tl.tab, &tab);
	if (s.prog) {
		const ProgSlot &ps = pa.slots[s.prog - 1u];
		const ProgScanDef sc = k_prog_script[ps.grey][prog_tile_scan(tl)];
		prog_tile_setup(ps, s, tl, blockIdx.x, sc, pa.fl, pa.after, nullptr, &pl);
		prog_pack_tile(&tab, s, tl, sc, reinterpret_cast<const int16_t *>(du_base + s.du_off), h, nwords, buf, uoff, &pl);
	} else {
		emit_pack_tile(&tab, s, tl, reinterpret_cast<const int16_t *>(du_base + s.du_off), h, nwords, buf, uoff);
	}
	if (h && threadIdx.x == 0) /* the previous tile's tail completes the first byte */
		buf[0] |= (s.prog ? pa.ctail[blockIdx.x - 1] : t_frag[blockIdx.x - 1] >> 8) << (32 - h);
	__syncthreads();
	/* each thread a contiguous run of the tile's bytes; a block scan of the stuffed sizes places the runs */
	const uint32_t per = (n_own + blockDim.x - 1) / blockDim.x;
	const uint32_t j0 = min(n_own, threadIdx.x * per), j1 = min(n_own, j0 + per);
	uint32_t c = j1 - j0;
	for (uint32_t j = j0; j < j1; ++j)
		c += lds_byte(buf, j) == 0xFFu;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t incl = wave_incl_scan(c, lane);
	if (lane == 63)
		part[wave] = incl;
	__syncthreads();
	uint32_t pos = incl - c;
	for (int w = 0; w < wave; ++w)
		pos += part[w];
	uint8_t *o = out + s.hlen + t_out[blockIdx.x] + pos;
	for (uint32_t j = j0; j < j1; ++j) {
		const uint32_t b = lds_byte(buf, j);
		*o++ = (uint8_t)b;
		if (b == 0xFFu)
			*o++ = 0;
	}
	if ((tl.pad & MIJ_TILE_ENDS) && s.prog) { /* the next scan's header behind the scan's stuffed bytes */
		const uint32_t q = (s.prog - 1u) * MIJ_PROG_SCANS + prog_tile_scan(tl) + 1u;
		uint8_t *m = out + s.hlen + t_out[blockIdx.x] + part[0] + part[1] + part[2] + part[3];
		for (uint32_t i = threadIdx.x; i < pa.hlen[q]; i += blockDim.x)
			m[i] = pa.hdr[(size_t)q * MIJ_PROG_HDR + i];
	} else if ((tl.pad & MIJ_TILE_ENDS) && threadIdx.x == 0) { /* the interval's marker, unstuffed, behind the tile's stuffed bytes */
		uint8_t *m = out + s.hlen + t_out[blockIdx.x] + part[0] + part[1] + part[2] + part[3];
		m[0] = 0xFF;
		m[1] = (uint8_t)(0xD0u + ((tl.pad >> 10) & 7u));
	}
}

/* ---- optimised Huffman tables */

/* the owner that counts the symbols: hist[4][256] in LDS */
struct LaneCounter {
	uint32_t *hist, *dcH, *acH;
	__device__ __forceinline__ void begin(bool luma)
	{
		dcH = hist + (luma ? 0 : 1) * 256;
		acH = hist + (luma ? 2 : 3) * 256;
	}
	__device__ __forceinline__ void dc(int n, uint32_t) { atomicAdd(&dcH[n & 255], 1u); }
	__device__ __forceinline__ void ac(int zrl, int sym, int, uint32_t)
	{
		if (zrl)
			atomicAdd(&acH[0xF0], (uint32_t)zrl);
		atomicAdd(&acH[sym & 255], 1u);
	}
	__device__ __forceinline__ void eob() { atomicAdd(&acH[0], 1u); }
};

/* per tile of an optimised slot: its symbols counted, freq[(s.tab - 1)][4][256] += (luma DC, chroma DC, luma AC, chroma AC) */
__global__ __launch_bounds__(256) void k_emit_hist(const EmitSlot *__restrict__ slots, const EmitTile *__restrict__ tiles, const uint8_t *__restrict__ du_base,
																	uint32_t *__restrict__ freq)
{
	__shared__ uint32_t hist[4 * 256];
	const EmitTile tl = tiles[blockIdx.x];
	const EmitSlot s = slots[tl.slot];
	const int16_t *du = reinterpret_cast<const int16_t *>(du_base + s.du_off);
	const int lane = threadIdx.x & 63;
	for (uint32_t i = threadIdx.x; i < 4 * 256; i += blockDim.x)
		hist[i] = 0;
	__syncthreads();
	emit_unit_loop(s, tl, du, [&](uint32_t, uint32_t u, UnitIn in) {
		LaneCounter c = {hist, nullptr, nullptr};
		emit_owner(s, in, u, lane, c);
	});
	__syncthreads();
	uint32_t *g = freq + (size_t)(s.tab - 1u) * (4 * 256);
	for (uint32_t i = threadIdx.x; i < 4 * 256; i += blockDim.x)
		if (hist[i])
			atomicAdd(&g[i], hist[i]);
}

/* the SOS segment behind the DHT segment (mjw_header), and a grey slot's (mjw_theader) */
__device__ const uint8_t k_emit_sos[14] = {0xFF, 0xDA, 0, 0xC, 3, 1, 0, 2, 0x11, 3, 0x11, 0, 0x3F, 0};
__device__ const uint8_t k_emit_sos1[10] = {0xFF, 0xDA, 0, 8, 1, 1, 0, 0, 0x3F, 0};
#define MIJ_EMIT_DHT_AT 177 /* the first byte behind the DHT segment's length in a three-component header */
#define MIJ_EMIT_DHT_AT1 106 /* ... in a grey header: one quantisation table, one component in SOF0 */

__device__ __forceinline__ uint64_t wave_min64(uint64_t v)
{
	for (int o = 32; o > 0; o >>= 1) {
		const uint64_t t = __shfl_xor(v, o, 64);
		v = t < v ? t : v;
	}
	return v;
}

/* Wave t of a workgroup of four builds table t from its 256 counts f by ITU-T T.81 K.2 as libjpeg's jpeg_gen_optimal_table does
 * (mjw_optimal_table, csrc/jpeg_write_host.c, is the same procedure on the host); k_emit_build and k_prog_build share it.  Lane l holds
 * the entries l, l + 64, l + 128, l + 192 and, lane 0, the pseudo-symbol 256 in registers.  A merge is two wave-wide argmins over
 * (count, largest index first) and one pass that gives every leaf of the two trees one more bit and the first tree's name -- the
 * leaves libjpeg reaches through its `others` chains.  Counts are uint32: a table holds at most 64 symbols per unit and
 * mij_enc_set_optimize / mij_enc_set_progressive refuse slots of more than 2^32 / 64 units, so no sum wraps.  Integer arithmetic only.
 * Out: bits[t][l] the number of codes of length l after K.3, first_code / first_pos Annex C's first code and first HUFFVAL position of each
 * length, nvals[t] the number of codes; pos[q] the HUFFVAL position of symbol lane + 64 * q (-1: no code), nv their number; *fail_p is
 * raised for a code above 32 bits before the shortening.  bits[t][0..33] and *fail_p are zero on entry, behind a barrier. */
__device__ __forceinline__ void emit_k2(const uint32_t *__restrict__ f, int lane, int t, uint32_t (*bits)[34], uint32_t (*first_code)[17],
													 uint32_t (*first_pos)[17], uint32_t *nvals, uint32_t *fail_p, int pos[4], uint32_t &nv)
{
	uint32_t &fail = *fail_p;
	uint32_t fr[5];
	int cs[5], grp[5];
#pragma unroll
	for (int q = 0; q < 5; ++q) {
		fr[q] = q < 4 ? f[lane + 64 * q] : (lane == 0 ? 1u : 0u);
		cs[q] = 0;
		grp[q] = lane + 64 * q;
	}
	for (;;) {
		uint64_t k1 = ~0ull, k2 = ~0ull;
#pragma unroll
		for (int q = 0; q < 5; ++q)
			if (fr[q]) {
				const uint64_t key = (uint64_t)fr[q] << 32 | (uint32_t)(511 - (lane + 64 * q)); /* smallest count, then largest index */
				k1 = key < k1 ? key : k1;
			}
		k1 = wave_min64(k1);
		const int c1 = 511 - (int)(uint32_t)k1;
#pragma unroll
		for (int q = 0; q < 5; ++q)
			if (fr[q] && lane + 64 * q != c1) {
				const uint64_t key = (uint64_t)fr[q] << 32 | (uint32_t)(511 - (lane + 64 * q));
				k2 = key < k2 ? key : k2;
			}
		k2 = wave_min64(k2);
		if (k2 == ~0ull)
			break;
		const int c2 = 511 - (int)(uint32_t)k2;
		const uint32_t sum = (uint32_t)(k1 >> 32) + (uint32_t)(k2 >> 32);
#pragma unroll
		for (int q = 0; q < 5; ++q) {
			const int i = lane + 64 * q;
			if (i == c1)
				fr[q] = sum;
			if (i == c2)
				fr[q] = 0;
			if (grp[q] == c1 || grp[q] == c2) {
				++cs[q];
				grp[q] = c1;
			}
		}
	}
	/* the lengths' counts (pseudo-symbol included); HUFFVAL position of each symbol: by unlimited length, then by value */
	bool deep = false;
#pragma unroll
	for (int q = 0; q < 5; ++q) {
		deep = deep || cs[q] > 32;
		if (cs[q] >= 1 && cs[q] <= 32)
			atomicAdd(&bits[t][cs[q]], 1u);
	}
	if (__ballot(deep) != 0 && lane == 0)
		atomicOr(&fail, 1u);
	pos[0] = pos[1] = pos[2] = pos[3] = -1;
	nv = 0;
	for (int l = 1; l <= 32; ++l)
#pragma unroll
		for (int q = 0; q < 4; ++q) {
			const uint64_t m = __ballot(cs[q] == l);
			if (cs[q] == l)
				pos[q] = (int)(nv + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)));
			nv += (uint32_t)__popcll(m);
		}
	__syncthreads();
	if (lane == 0 && !fail) { /* K.3: lengths above 16 shortened pairwise; the pseudo-symbol's code removed; Annex C's first codes */
		uint32_t *b = bits[t];
		for (int i = 32; i > 16; --i)
			while (b[i] > 0) {
				int j = i - 2;
				while (j > 0 && b[j] == 0)
					--j;
				b[i] -= 2;
				++b[i - 1];
				b[j + 1] += 2;
				--b[j];
			}
		int i = 16;
		while (i > 0 && b[i] == 0)
			--i;
		if (i > 0)
			--b[i];
		uint32_t code = 0, p = 0;
		for (int l = 1; l <= 16; ++l) {
			first_code[t][l] = code;
			first_pos[t][l] = p;
			code = (code + b[l]) << 1;
			p += b[l];
		}
		nvals[t] = p;
	}
	__syncthreads();
}

/* One workgroup per optimised slot k (slot opt_slots[k], counts freq[k], tables tabs[k + 1]): the four tables by emit_k2, the slot's EmitTables
 * entry, its DHT segment and header length */
__global__ __launch_bounds__(256) void k_emit_build(EmitSlot *__restrict__ slots, EmitTile *__restrict__ tiles, const uint32_t *__restrict__ opt_slots,
																	 const uint32_t *__restrict__ freq, EmitTables *__restrict__ tabs, uint8_t *__restrict__ hdrs,
																	 uint32_t *__restrict__ opt_ok)
{
	__shared__ uint32_t bits[4][34], first_code[4][17], first_pos[4][17], nvals[4];
	__shared__ uint32_t fail;
	const int lane = threadIdx.x & 63, t = threadIdx.x >> 6;
	const uint32_t k = blockIdx.x, slot = opt_slots[k];
	if (threadIdx.x == 0)
		fail = 0;
	if (lane < 34)
		bits[t][lane] = 0;
	__syncthreads();
	int pos[4];
	uint32_t nv;
	emit_k2(freq + (size_t)k * (4 * 256) + t * 256, lane, t, bits, first_code, first_pos, nvals, &fail, pos, nv);
	/* a slot without chroma (dpm == ny) carries the two luma tables only, in the shorter header */
	const bool grey = slots[slot].dpm == slots[slot].ny;
	/* libjpeg's framing: a second DQT segment in front (4 bytes more), and every table in a DHT segment of its own (4 bytes more each) */
	const uint32_t lj = slots[slot].lj ? 4u : 0u;
	const uint32_t dht_at = (grey ? MIJ_EMIT_DHT_AT1 : MIJ_EMIT_DHT_AT + lj), sos_len = grey ? 10u : 14u;
	/* behind the DHT segment: the DRI segment of a slot with a restart interval, then SOS */
	const uint32_t ri = slots[slot].ri, tail = sos_len + (ri ? 6u : 0u);
	const uint32_t hlen = grey ? dht_at + 2u * 17u + lj + nvals[0] + nvals[2] + tail : dht_at + 4u * 17u + 3u * lj + nvals[0] + nvals[1] + nvals[2] + nvals[3] + tail;
	const bool ok = !fail && hlen <= MIJ_EMIT_HDR && nvals[t] == nv;
	const bool all_ok = __syncthreads_and(ok) != 0;
	const uint32_t tile0 = slots[slot].first_tile, ntile = slots[slot].n_tiles;
	for (uint32_t i = threadIdx.x; i < ntile; i += blockDim.x)
		tiles[tile0 + i].tab = all_ok ? k + 1 : 0u;
	if (all_ok) {
		/* the DHT segment holds the tables in mjw_header's order: luma DC, luma AC, chroma DC, chroma AC */
		const uint32_t before = t == 0 ? 0u : (t == 2 ? 17u + lj + nvals[0] : (t == 1 ? 34u + 2u * lj + nvals[0] + nvals[2] : 51u + 3u * lj + nvals[0] + nvals[2] + nvals[1]));
		uint8_t *h = hdrs + (size_t)slots[slot].hdr * MIJ_EMIT_HDR, *seg = h + dht_at + before;
		EmitTables *T = tabs + k + 1;
		const bool in_dht = !grey || t == 0 || t == 2; /* the code tables are written for all four: a grey slot never looks its chroma tables up */
		if (lane == 0 && in_dht)
			seg[0] = (uint8_t)(t == 0 ? 0x00 : (t == 2 ? 0x10 : (t == 1 ? 0x01 : 0x11)));
		if (lane < 4 && in_dht && lj) { /* the table's own FF C4 and length */
			const uint32_t head = 0xFFu | 0xC4u << 8 | ((19u + nvals[t]) >> 8) << 16 | ((19u + nvals[t]) & 0xFFu) << 24;
			seg[lane - 4] = (uint8_t)(head >> (8 * lane));
		}
		if (lane < 16 && in_dht)
			seg[1 + lane] = (uint8_t)bits[t][lane + 1];
#pragma unroll
		for (int q = 0; q < 4; ++q) {
			uint32_t code = 0, len = 0;
			if (pos[q] >= 0) {
				for (int l = 1; l <= 16; ++l)
					if ((uint32_t)pos[q] >= first_pos[t][l] && (uint32_t)pos[q] < first_pos[t][l] + bits[t][l]) {
						len = (uint32_t)l;
						code = first_code[t][l] + (uint32_t)pos[q] - first_pos[t][l];
					}
				if (in_dht)
					seg[17 + pos[q]] = (uint8_t)(lane + 64 * q);
			}
			T->code[t][lane + 64 * q] = (uint16_t)code;
			T->len[t][lane + 64 * q] = (uint8_t)len;
		}
		if (t == 3 && (uint32_t)lane < sos_len)
			h[hlen - sos_len + lane] = grey ? k_emit_sos1[lane] : k_emit_sos[lane];
		if (t == 2 && ri && lane < 6) {
			const uint32_t dri = 0xFFu | 0xDDu << 8 | 4u << 24; /* FF DD 00 04 */
			h[hlen - tail + lane] = (uint8_t)(lane < 4 ? dri >> (8 * lane) : (lane == 4 ? ri >> 8 : ri));
		}
		if (threadIdx.x == 0) {
			if (!lj) {
				h[dht_at - 2] = (uint8_t)((hlen - tail - (dht_at - 2)) >> 8);
				h[dht_at - 1] = (uint8_t)((hlen - tail - (dht_at - 2)) & 0xFFu);
			}
			slots[slot].hlen = hlen;
			opt_ok[k] = 1;
		}
	} else if (threadIdx.x == 0) { /* the plain tables and the plain header, which the upload left in place */
		opt_ok[k] = 0; /* hlen is still the plain header's, as the upload wrote it */
	}
}

/* One workgroup per (progressive slot, scan): the scan's tables by emit_k2 from the counts k_prog_hist left -- DC tables 0 and 1 in the first
 * DC scan, the AC table in wave 2 of an AC scan, none in the DC refinement -- into EmitTables entry tab0 + scan, which the scan's tiles are
 * pointed at; the scan's header: a DHT segment per table, then SOS.  The first scan's goes behind the frame header of the slot's header
 * (EmitSlot.hlen grows by it), the others into phdr for k_emit_write to place between the scans.  A table K.2 refuses raises p_flag. */
__global__ __launch_bounds__(256) void k_prog_build(EmitSlot *__restrict__ slots, EmitTile *__restrict__ tiles, const ProgSlot *__restrict__ pslots,
																	 const uint32_t *__restrict__ freq, EmitTables *__restrict__ tabs, uint8_t *__restrict__ hdrs,
																	 uint8_t *__restrict__ phdr, uint32_t *__restrict__ phlen, uint32_t *__restrict__ p_flag)
{
	__shared__ uint32_t bits[4][34], first_code[4][17], first_pos[4][17], nvals[4];
	__shared__ uint32_t fail;
	const int lane = threadIdx.x & 63, t = threadIdx.x >> 6;
	const uint32_t q = blockIdx.x, scan = q % MIJ_PROG_SCANS;
	const ProgSlot &ps = pslots[q / MIJ_PROG_SCANS];
	if (scan >= ps.nscan)
		return;
	const ProgScanDef sc = k_prog_script[ps.grey][scan];
	if (threadIdx.x == 0)
		fail = 0;
	if (lane < 34)
		bits[t][lane] = 0;
	__syncthreads();
	int pos[4];
	uint32_t nv;
	emit_k2(freq + (size_t)q * (4 * 256) + t * 256, lane, t, bits, first_code, first_pos, nvals, &fail, pos, nv);
	const bool dc = sc.ss == 0, grey = ps.grey != 0;
	const bool used = dc ? !sc.ah && (t == 0 || (t == 1 && !grey)) : t == 2;
	const bool all_ok = __syncthreads_and(!fail && nvals[t] == nv) != 0;
	const uint32_t dht = dc ? (sc.ah ? 0u : 21u + nvals[0] + (grey ? 0u : 21u + nvals[1])) : 21u + nvals[2];
	const uint32_t sos_len = 8u + 2u * sc.ncomp, hl = dht + sos_len;
	uint8_t *h = scan == 0 ? hdrs + (size_t)slots[ps.slot].hdr * MIJ_EMIT_HDR + ps.frame_len : phdr + (size_t)q * MIJ_PROG_HDR;
	for (uint32_t i = ps.tile0[scan] + threadIdx.x; i < ps.tile0[scan + 1]; i += blockDim.x)
		tiles[i].tab = ps.tab0 + scan;
	if (threadIdx.x == 0) {
		phlen[q] = hl;
		if (scan == 0)
			slots[ps.slot].hlen = ps.frame_len + hl;
		if (!all_ok)
			p_flag[ps.slot] = 1u;
	}
	if (!all_ok)
		return;
	EmitTables *T = tabs + ps.tab0 + scan;
	uint8_t *seg = h + (dc && t == 1 ? 21u + nvals[0] : 0u);
	if (used) {
		const uint32_t head = 0xFFu | 0xC4u << 8 | ((19u + nv) >> 8) << 16 | ((19u + nv) & 0xFFu) << 24; /* FF C4, the segment's length */
		if (lane < 4)
			seg[lane] = (uint8_t)(head >> (8 * lane));
		if (lane == 4)
			seg[4] = (uint8_t)(dc ? t : 0x10 | (sc.comp ? 1 : 0));
		if (lane < 16)
			seg[5 + lane] = (uint8_t)bits[t][lane + 1];
	}
#pragma unroll
	for (int qq = 0; qq < 4; ++qq) {
		uint32_t code = 0, len = 0;
		if (pos[qq] >= 0) {
			for (int l = 1; l <= 16; ++l)
				if ((uint32_t)pos[qq] >= first_pos[t][l] && (uint32_t)pos[qq] < first_pos[t][l] + bits[t][l]) {
					len = (uint32_t)l;
					code = first_code[t][l] + (uint32_t)pos[qq] - first_pos[t][l];
				}
			if (used)
				seg[21 + pos[qq]] = (uint8_t)(lane + 64 * qq);
		}
		T->code[t][lane + 64 * qq] = (uint16_t)code;
		T->len[t][lane + 64 * qq] = (uint8_t)len;
	}
	if (t == 3 && (uint32_t)lane < sos_len) { /* FF DA, length, components with their table byte, Ss, Se, Ah Al */
		const uint32_t nc = sc.ncomp, i = (uint32_t)lane;
		uint32_t b;
		if (i < 5)
			b = i == 0 ? 0xFFu : (i == 1 ? 0xDAu : (i == 2 ? 0u : (i == 3 ? 6u + 2u * nc : nc)));
		else if (i < 5 + 2 * nc) {
			const uint32_t c = dc ? (i - 5) >> 1 : sc.comp;
			/* Td only in the first DC scan, Ta only in AC scans */
			b = (i - 5) & 1u ? (dc ? (sc.ah || c == 0 ? 0u : 0x10u) : (c ? 1u : 0u)) : c + 1u;
		} else {
			const uint32_t k = i - 5 - 2 * nc;
			b = k == 0 ? sc.ss : (k == 1 ? sc.se : (uint32_t)sc.ah << 4 | sc.al);
		}
		h[dht + i] = (uint8_t)b;
	}
}

/* ---- encoder slots with device pixels: the pixel arena's padded packed-RGB rows gathered from the caller's tensor (the channel
 * rule and edge replication of enc_stage_rows).  One workgroup per 4 rows; a thread makes 4 pixels = 3 aligned words. */
struct EncGather {
	const uint8_t *src;
	int64_t row_pitch, plane_pitch;
	int32_t layout, width, height, comp;
	int32_t pad_w, pad;
	uint64_t pix_off;
};
#define MIJ_GATHER_ROWS 4

__global__ __launch_bounds__(256) void k_enc_gather(const EncGather *__restrict__ gs, const WorkIdct *__restrict__ work, uint8_t *__restrict__ pix)
{
	const WorkIdct wk = work[blockIdx.x];
	const EncGather g = gs[wk.img];
	const uint32_t y0 = wk.first, rows = min((uint32_t)MIJ_GATHER_ROWS, (uint32_t)g.height - y0), groups = (uint32_t)g.pad_w / 4;
	const int og = g.comp > 2 ? 1 : 0, ob = g.comp > 2 ? 2 : 0;
	const bool chw = g.layout == 1;
	const int64_t sg = chw ? og * g.plane_pitch : og, sb = chw ? ob * g.plane_pitch : ob, sx = chw ? 1 : g.comp;
	for (uint32_t idx = threadIdx.x; idx < rows * groups; idx += blockDim.x) {
		const uint32_t y = y0 + idx / groups, x0 = (idx % groups) * 4;
		const uint8_t *row = g.src + (int64_t)y * g.row_pitch;
		uint32_t px[4];
		for (int j = 0; j < 4; ++j) {
			const int x = min((int)x0 + j, g.width - 1);
			const uint8_t *p = row + (int64_t)x * sx;
			px[j] = (uint32_t)p[0] | (uint32_t)p[sg] << 8 | (uint32_t)p[sb] << 16;
		}
		uint32_t *d = reinterpret_cast<uint32_t *>(pix + g.pix_off + (size_t)y * (size_t)g.pad_w * 3 + (size_t)x0 * 3);
		d[0] = px[0] | px[1] << 24;
		d[1] = px[1] >> 8 | px[2] << 16;
		d[2] = px[2] >> 16 | px[3] << 8;
	}
}

/* ---- device pixels held as float16 / bfloat16 / float32 (mij_enc_add_device_float): the same padded packed-RGB rows, every element
 * de-normalised by the contract of include/mij.h on the way.  The same work list and the same output as k_enc_gather: one workgroup
 * per MIJ_GATHER_ROWS rows, a thread makes 4 pixels = 3 aligned words.  A thread's 4 pixels are 4 consecutive elements of each plane
 * (planar: CHW, and grey in either layout) or 4*comp consecutive elements (interleaved): each run of 4 elements is one 8-byte
 * (16-bit types) or 16-byte (float32) load where its address is so aligned and the group lies inside the picture, and 4 element
 * loads otherwise -- the right-edge group, whose x clamps to width-1, and rows that base pointer, row pitch or plane pitch leave
 * misaligned.  x0 is a multiple of 4, so a row (of one plane) is aligned or not as a whole and a wavefront diverges at the edge
 * group only.  Both paths fetch the same elements. */
struct EncGatherF {
	EncGather g; /* src and the pitches count elements of the slot's dtype */
	float scale[4], bias[4];
};

struct GatherF16 {
	typedef uint16_t raw;
	static __device__ __forceinline__ float widen(uint16_t v) { return (float)__builtin_bit_cast(_Float16, v); }
};
struct GatherBF16 {
	typedef uint16_t raw;
	static __device__ __forceinline__ float widen(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }
};
struct GatherF32 {
	typedef uint32_t raw;
	static __device__ __forceinline__ float widen(uint32_t v) { return __uint_as_float(v); }
};

/* 4 elements with one load.  Native vector types: as a struct of four words the load falls apart into element loads, which the
 * compiler then merges with the element path's */
typedef uint32_t gather_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t gather_u32x4 __attribute__((ext_vector_type(4)));
static __device__ __forceinline__ void gather_load4(const uint16_t *p, uint16_t *r)
{
	const gather_u32x2 v = *reinterpret_cast<const gather_u32x2 *>(p);
	r[0] = (uint16_t)v.x, r[1] = (uint16_t)(v.x >> 16), r[2] = (uint16_t)v.y, r[3] = (uint16_t)(v.y >> 16);
}
static __device__ __forceinline__ void gather_load4(const uint32_t *p, uint32_t *r)
{
	const gather_u32x4 v = *reinterpret_cast<const gather_u32x4 *>(p);
	r[0] = v.x, r[1] = v.y, r[2] = v.z, r[3] = v.w;
}

/* the contract's u for the widened element x: two roundings, never a fused multiply-add */
static __device__ __forceinline__ uint32_t gather_denorm(float x, float scale, float bias)
{
#pragma clang fp contract(off)
	float t = __fadd_rn(__fmul_rn(x, scale), bias);
	t = t > 0.0f ? t : 0.0f;     /* fmaxf(t, 0.0f), spelled out: NaN fails the comparison and becomes 0 */
	t = t < 255.0f ? t : 255.0f; /* fminf(t, 255.0f) */
	return (uint32_t)rintf(t);   /* round half to even */
}

/* SX: elements from one pixel to the next (1: planar, channel c lies c * plane_pitch further; else interleaved, channel c is element c
 * of the pixel); NCH: channels read (1: grey, the picture's first channel in r, g and b; 3) */
template <typename D, int SX, int NCH>
static __device__ __forceinline__ void gather_float_rows(const EncGatherF &G, uint32_t y0, uint32_t rows, uint8_t *__restrict__ pix)
{
	typedef typename D::raw R;
	const EncGather &g = G.g;
	const R *src = reinterpret_cast<const R *>(g.src);
	const uint32_t groups = (uint32_t)g.pad_w / 4;
	const uintptr_t vmask = 4 * sizeof(R) - 1;
	for (uint32_t idx = threadIdx.x; idx < rows * groups; idx += blockDim.x) {
		const uint32_t y = y0 + idx / groups, x0 = (idx % groups) * 4;
		const R *row = src + (int64_t)y * g.row_pitch;
		const bool inside = x0 + 4 <= (uint32_t)g.width;
		R e[4][NCH];
		if (SX == 1) {
#pragma unroll
			for (int c = 0; c < NCH; ++c) {
				const R *plane = row + (int64_t)c * g.plane_pitch;
				if (inside && ((uintptr_t)(plane + x0) & vmask) == 0) {
					R r[4];
					gather_load4(plane + x0, r);
#pragma unroll
					for (int j = 0; j < 4; ++j)
						e[j][c] = r[j];
				} else {
#pragma unroll
					for (int j = 0; j < 4; ++j)
						e[j][c] = plane[min((int)x0 + j, g.width - 1)];
				}
			}
		} else {
			const R *p = row + (int64_t)x0 * SX;
			if (inside && ((uintptr_t)p & vmask) == 0) {
				R r[4 * SX];
#pragma unroll
				for (int k = 0; k < SX; ++k)
					gather_load4(p + 4 * k, r + 4 * k);
#pragma unroll
				for (int j = 0; j < 4; ++j)
#pragma unroll
					for (int c = 0; c < NCH; ++c)
						e[j][c] = r[j * SX + c];
			} else {
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					const R *q = row + (int64_t)min((int)x0 + j, g.width - 1) * SX;
#pragma unroll
					for (int c = 0; c < NCH; ++c)
						e[j][c] = q[c];
				}
			}
		}
		uint32_t px[4];
#pragma unroll
		for (int j = 0; j < 4; ++j) {
			const uint32_t r = gather_denorm(D::widen(e[j][0]), G.scale[0], G.bias[0]);
			if constexpr (NCH == 3)
				px[j] = r | gather_denorm(D::widen(e[j][1]), G.scale[1], G.bias[1]) << 8 | gather_denorm(D::widen(e[j][2]), G.scale[2], G.bias[2]) << 16;
			else
				px[j] = r * 0x010101u;
		}
		uint32_t *d = reinterpret_cast<uint32_t *>(pix + g.pix_off + (size_t)y * (size_t)g.pad_w * 3 + (size_t)x0 * 3);
		d[0] = px[0] | px[1] << 24;
		d[1] = px[1] >> 8 | px[2] << 16;
		d[2] = px[2] >> 16 | px[3] << 8;
	}
}

template <typename D>
__global__ __launch_bounds__(256) void k_enc_gather_float(const EncGatherF *__restrict__ gs, const WorkIdct *__restrict__ work, uint8_t *__restrict__ pix)
{
	const WorkIdct wk = work[blockIdx.x];
	const EncGatherF G = gs[wk.img];
	const uint32_t y0 = wk.first, rows = min((uint32_t)MIJ_GATHER_ROWS, (uint32_t)G.g.height - y0);
	const int comp = G.g.comp;
	if (G.g.layout == 1 || comp == 1) { /* planar; the alpha plane of comp 2 and 4 is never read */
		if (comp > 2)
			gather_float_rows<D, 1, 3>(G, y0, rows, pix);
		else
			gather_float_rows<D, 1, 1>(G, y0, rows, pix);
	} else if (comp == 2) {
		gather_float_rows<D, 2, 1>(G, y0, rows, pix);
	} else if (comp == 3) {
		gather_float_rows<D, 3, 3>(G, y0, rows, pix);
	} else {
		gather_float_rows<D, 4, 3>(G, y0, rows, pix);
	}
}

/* ---- plane slots with device planes (mij_enc_add_device_planes; include/mij_host.h, PLANE ENCODING): each plane into the slot's share of
 * the pixel arena as planar rows padded to whole MCUs of its component -- the edge rule (the plane's own last column and row repeated),
 * the flip, the de-interleaving of NV12 / NV21 / packed layouts (x_pitch) and the range conversion all happen here, so the strip kernels
 * meet aligned rows and need no edge code.  k_enc_gather's work list: one workgroup per MIJ_PGATHER_ROWS staged rows of one plane; a
 * thread makes runs of 8 samples = one aligned 8-byte store.  Where x_pitch is 1 and the run lies inside the plane it is one 8-byte load
 * when its address is so aligned, two 4-byte loads when it is 4-aligned, and element loads otherwise (the edge run, other pitches). */
struct EncGatherP {
	const uint8_t *src[3];
	int64_t row_pitch[3], x_pitch[3];
	int32_t w[3], h[3];         /* each plane's own size */
	int32_t pad_w[3], pad_h[3]; /* its staged size: multiples of 8 */
	uint64_t dst_off[3];        /* where its staged rows begin in the pixel arena */
	int32_t flip, convert;
	float scale[3], bias[3];
};
#define MIJ_PGATHER_ROWS 8

__global__ __launch_bounds__(256) void k_enc_gather_planes(const EncGatherP *__restrict__ gs, const WorkIdct *__restrict__ work, uint8_t *__restrict__ pix)
{
	const WorkIdct wk = work[blockIdx.x];
	const EncGatherP &g = gs[wk.img];
	const int c = (int)wk.comp;
	const uint8_t *src = g.src[c];
	const int64_t rp = g.row_pitch[c], xp = g.x_pitch[c];
	const int w = g.w[c], h = g.h[c];
	const uint32_t y0 = wk.first, groups = (uint32_t)g.pad_w[c] / 8; /* pad_h is a multiple of MIJ_PGATHER_ROWS */
	const bool cvt = g.convert != 0;
	const float scale = g.scale[c], bias = g.bias[c];
	for (uint32_t idx = threadIdx.x; idx < MIJ_PGATHER_ROWS * groups; idx += blockDim.x) {
		const uint32_t y = y0 + idx / groups, x0 = (idx % groups) * 8;
		const int cy = min((int)y, h - 1);
		const uint8_t *row = src + (int64_t)(g.flip ? h - 1 - cy : cy) * rp;
		uint32_t lo, hi;
		const uint8_t *p = row + x0;
		if (xp == 1 && x0 + 8 <= (uint32_t)w && ((uintptr_t)p & 3) == 0) {
			if (((uintptr_t)p & 7) == 0) {
				const gather_u32x2 v = *reinterpret_cast<const gather_u32x2 *>(p);
				lo = v.x, hi = v.y;
			} else {
				lo = *reinterpret_cast<const uint32_t *>(p), hi = *reinterpret_cast<const uint32_t *>(p + 4);
			}
		} else {
			lo = hi = 0;
#pragma unroll
			for (int k = 0; k < 8; ++k) {
				const uint32_t v = row[(int64_t)min((int)x0 + k, w - 1) * xp];
				if (k < 4)
					lo |= v << (8 * k);
				else
					hi |= v << (8 * (k - 4));
			}
		}
		if (cvt) {
			uint32_t a = 0, b = 0;
#pragma unroll
			for (int k = 0; k < 4; ++k) {
				a |= gather_denorm((float)((lo >> (8 * k)) & 255u), scale, bias) << (8 * k);
				b |= gather_denorm((float)((hi >> (8 * k)) & 255u), scale, bias) << (8 * k);
			}
			lo = a, hi = b;
		}
		*reinterpret_cast<gather_u32x2 *>(pix + g.dst_off[c] + (size_t)y * (size_t)g.pad_w[c] + x0) = (gather_u32x2){lo, hi};
	}
}
