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
 */
#pragma once

#define MIJ_EMIT_TILE 128
#define MIJ_EMIT_HDR 607 /* MJW_HEADER_BYTES */
/* most bits a unit within the writer's ranges takes: chroma DC 11 + 11, 63 AC symbols of 16 + 10, the 7 fill bits */
#define MIJ_EMIT_MAX_DU_BITS (22 + 63 * 26 + 7)
#define MIJ_EMIT_LDS_WORDS ((MIJ_EMIT_TILE * MIJ_EMIT_MAX_DU_BITS + 7 + 31) / 32 + 1)

struct EmitTables {
	uint16_t code[4][256]; /* luma DC, chroma DC, luma AC, chroma AC */
	uint8_t len[4][256];
};

struct EmitSlot {
	uint64_t du_off; /* bytes into the data-unit arena */
	uint32_t n_du, dpm; /* units; units per MCU: 6 (4:2:0) or 3 (4:4:4) */
	uint32_t first_tile, n_tiles;
	uint32_t hdr, pad; /* header of the slot: hdrs + hdr * MIJ_EMIT_HDR */
};

struct EmitTile {
	uint32_t slot, first; /* the tile's first unit in its slot */
};

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

/* What lane `lane` emits for unit u of a slot: zrl ZRL codes, then sym, then extra (EOB and / or fill).  Every lane of the wave
 * must call it for the same unit (ballot). */
struct LaneBits {
	uint32_t sym, extra, zrl_code;
	int sym_len, extra_len, zrl_len, zrl;
	__device__ int total() const { return zrl * zrl_len + sym_len + extra_len; }
};
struct UnitIn {
	int v, pred; /* this lane's coefficient; the DC predictor (lane 0) */
};
/* the loads of unit u (issued a unit ahead of its use: emit_units) */
__device__ __forceinline__ UnitIn emit_load(const EmitSlot &s, const int16_t *__restrict__ du, uint32_t u, int lane)
{
	const uint32_t m = u / s.dpm, p = u - m * s.dpm;
	long prev = -1; /* the unit whose DC predicts this one's: the previous unit of the component in MCU order */
	if (s.dpm == 6u)
		prev = (p > 0 && p < 4) ? (long)u - 1 : (m > 0 ? (long)u - (p < 4 ? 3 : 6) : -1);
	else
		prev = m > 0 ? (long)u - 3 : -1;
	UnitIn in;
	in.v = du[(size_t)u * 64 + lane];
	in.pred = lane == 0 && prev >= 0 ? (int)du[(size_t)prev * 64] : 0;
	return in;
}
__device__ __forceinline__ void emit_lane(const EmitTables *__restrict__ T, const EmitSlot &s, UnitIn in, uint32_t u, int lane, LaneBits &L)
{
	const uint32_t m = u / s.dpm, p = u - m * s.dpm;
	const bool luma = p < (s.dpm == 6u ? 4u : 1u);
	const int v = in.v;
	const uint64_t nz = __ballot(v != 0) & ~1ull;
	const int dc = luma ? 0 : 1, ac = luma ? 2 : 3;
	L.sym = L.extra = L.zrl_code = 0;
	L.sym_len = L.extra_len = L.zrl_len = L.zrl = 0;
	if (lane == 0) {
		const int diff = v - in.pred;
		if (diff == 0) {
			L.sym = T->code[dc][0];
			L.sym_len = T->len[dc][0];
		} else {
			uint32_t bits;
			const int n = emit_mag(diff, bits);
			L.sym = ((uint32_t)T->code[dc][n] << n) | bits;
			L.sym_len = T->len[dc][n] + n;
		}
	} else if (v != 0) {
		const uint64_t below = nz & ((1ull << lane) - 1ull);
		const int last = below ? 63 - __clzll((long long)below) : 0;
		const int run = lane - last - 1;
		uint32_t bits;
		const int n = emit_mag(v, bits), sym = ((run & 15) << 4) + n;
		L.zrl = run >> 4;
		L.zrl_code = T->code[ac][0xF0];
		L.zrl_len = T->len[ac][0xF0];
		L.sym = ((uint32_t)T->code[ac][sym & 255] << n) | bits;
		L.sym_len = T->len[ac][sym & 255] + n;
	}
	if (lane == 63) {
		if (v == 0) {
			L.extra = T->code[ac][0];
			L.extra_len = T->len[ac][0];
		}
		if (u + 1 == s.n_du) { /* the slot's last unit: fill to a byte boundary with ones */
			L.extra = (L.extra << 7) | 0x7Fu;
			L.extra_len += 7;
		}
	}
}

/* f(j, LaneBits) for the units j = wave, wave + 4, ... < n of a tile (first unit `first`), the next unit's loads in flight */
template <typename F>
__device__ __forceinline__ void emit_units(const EmitTables *__restrict__ T, const EmitSlot &s, const int16_t *__restrict__ du, uint32_t first, uint32_t n,
														 F f)
{
	const int lane = threadIdx.x & 63;
	uint32_t j = threadIdx.x >> 6;
	if (j >= n)
		return;
	UnitIn in = emit_load(s, du, first + j, lane);
	for (; j < n; j += 4) {
		UnitIn next = in;
		if (j + 4 < n)
			next = emit_load(s, du, first + j + 4, lane);
		LaneBits L;
		emit_lane(T, s, in, first + j, lane, L);
		f(j, L);
		in = next;
	}
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

/* Packs tile tl's bits into buf from bit h on (buf zeroed here; nwords of it are used).  uoff: MIJ_EMIT_TILE + 1 words of LDS. */
__device__ void emit_pack_tile(const EmitTables *__restrict__ T, const EmitSlot &s, const EmitTile &tl, const int16_t *__restrict__ du, uint32_t h,
										 uint32_t nwords, uint32_t *buf, uint32_t *uoff)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t n = min((uint32_t)MIJ_EMIT_TILE, s.n_du - tl.first);
	for (uint32_t i = threadIdx.x; i < nwords; i += blockDim.x)
		buf[i] = 0;
	emit_units(T, s, du, tl.first, n, [&](uint32_t j, const LaneBits &L) {
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
	emit_units(T, s, du, tl.first, n, [&](uint32_t j, const LaneBits &L) {
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
																  const EmitTables *__restrict__ T, const uint8_t *__restrict__ du_base, uint32_t *__restrict__ t_bits)
{
	__shared__ uint32_t part[4];
	__shared__ EmitTables tab;
	const EmitTile tl = tiles[blockIdx.x];
	const EmitSlot s = slots[tl.slot];
	const int16_t *du = reinterpret_cast<const int16_t *>(du_base + s.du_off);
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t n = min((uint32_t)MIJ_EMIT_TILE, s.n_du - tl.first);
	emit_tables_to_lds(T, &tab);
	uint32_t acc = 0;
	emit_units(&tab, s, du, tl.first, n, [&](uint32_t, const LaneBits &L) { acc += wave_sum((uint32_t)L.total()); });
	if (lane == 0)
		part[wave] = acc;
	__syncthreads();
	if (threadIdx.x == 0)
		t_bits[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

/* one wave per slot: each tile's bit offset in its slot */
__global__ __launch_bounds__(256) void k_emit_scan(const EmitSlot *__restrict__ slots, uint32_t n_slots, const uint32_t *__restrict__ t_bits,
																	uint64_t *__restrict__ t_boff)
{
	const int lane = threadIdx.x & 63;
	const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (i >= n_slots)
		return;
	const EmitSlot s = slots[i];
	uint64_t base = 0;
	for (uint32_t t0 = 0; t0 < s.n_tiles; t0 += 64) {
		const uint32_t t = t0 + (uint32_t)lane;
		const uint32_t v = t < s.n_tiles ? t_bits[s.first_tile + t] : 0u;
		const uint32_t incl = wave_incl_scan(v, lane);
		if (t < s.n_tiles)
			t_boff[s.first_tile + t] = base + incl - v;
		base += __shfl(incl, 63, 64);
	}
}

/* per tile: the 0xFF bytes among those whose 8 bits all lie in the tile, and the head / tail fragments (t_frag = head | tail << 8) */
__global__ __launch_bounds__(256) void k_emit_count(const EmitSlot *__restrict__ slots, const EmitTile *__restrict__ tiles,
																	 const EmitTables *__restrict__ T, const uint8_t *__restrict__ du_base, const uint32_t *__restrict__ t_bits,
																	 const uint64_t *__restrict__ t_boff, uint32_t *__restrict__ t_ff, uint32_t *__restrict__ t_frag)
{
	__shared__ uint32_t buf[MIJ_EMIT_LDS_WORDS];
	__shared__ uint32_t uoff[MIJ_EMIT_TILE + 1];
	__shared__ uint32_t part[4];
	__shared__ EmitTables tab;
	const EmitTile tl = tiles[blockIdx.x];
	const EmitSlot s = slots[tl.slot];
	const uint64_t b0 = t_boff[blockIdx.x], b1 = b0 + t_bits[blockIdx.x];
	const uint32_t h = (uint32_t)(b0 & 7u), n_own = (uint32_t)((b1 >> 3) - (b0 >> 3));
	const uint32_t nwords = (uint32_t)((h + (b1 - b0) + 31) / 32);
	if (nwords > MIJ_EMIT_LDS_WORDS - 1) { /* only units outside the writer's ranges get here: the slot is refused (k_emit_stuff) */
		if (threadIdx.x == 0) {
			t_ff[blockIdx.x] = ~0u;
			t_frag[blockIdx.x] = 0;
		}
		return;
	}
	emit_tables_to_lds(T, &tab);
	emit_pack_tile(&tab, s, tl, reinterpret_cast<const int16_t *>(du_base + s.du_off), h, nwords, buf, uoff);
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
__global__ __launch_bounds__(256) void k_emit_stuff(const EmitSlot *__restrict__ slots, uint32_t n_slots, const uint32_t *__restrict__ t_bits,
																	 const uint64_t *__restrict__ t_boff, const uint32_t *__restrict__ t_ff, const uint32_t *__restrict__ t_frag,
																	 uint64_t *__restrict__ t_out, uint64_t *__restrict__ s_ent)
{
	const int lane = threadIdx.x & 63;
	const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (i >= n_slots)
		return;
	const EmitSlot s = slots[i];
	uint64_t base = 0;
	bool bad = false;
	for (uint32_t t0 = 0; t0 < s.n_tiles; t0 += 64) {
		const uint32_t t = t0 + (uint32_t)lane, g = s.first_tile + t;
		uint32_t v = 0;
		if (t < s.n_tiles) {
			const uint64_t b0 = t_boff[g], b1 = b0 + t_bits[g];
			const uint32_t h = (uint32_t)(b0 & 7u), ff = t_ff[g];
			if (ff == ~0u) {
				bad = true;
			} else {
				v = (uint32_t)((b1 >> 3) - (b0 >> 3)) + ff;
				if (h && t > 0) { /* the byte shared with the previous tile */
					const uint32_t byte = ((t_frag[g - 1] >> 8) << (8 - h)) | (t_frag[g] & 0xFFu);
					v += byte == 0xFFu;
				}
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
__global__ __launch_bounds__(1024) void k_emit_place(uint32_t n_slots, const uint64_t *__restrict__ s_ent, uint64_t cap, EmitResult *__restrict__ res)
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
		const uint64_t len = i < n_slots && !bad ? MIJ_EMIT_HDR + ent + 2 : 0;
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
																	 const uint64_t *__restrict__ t_out, const EmitResult *__restrict__ res, uint8_t *__restrict__ arena)
{
	__shared__ uint32_t buf[MIJ_EMIT_LDS_WORDS];
	__shared__ uint32_t uoff[MIJ_EMIT_TILE + 1];
	__shared__ uint32_t part[4];
	__shared__ EmitTables tab;
	const EmitTile tl = tiles[blockIdx.x];
	const EmitResult r = res[tl.slot];
	if (r.off == ~0ull)
		return;
	const EmitSlot s = slots[tl.slot];
	uint8_t *out = arena + r.off;
	if (tl.first == 0)
		for (uint32_t i = threadIdx.x; i < MIJ_EMIT_HDR; i += blockDim.x)
			out[i] = hdrs[(size_t)s.hdr * MIJ_EMIT_HDR + i];
	if (tl.first + MIJ_EMIT_TILE >= s.n_du && threadIdx.x == 0) {
		out[r.len - 2] = 0xFF;
		out[r.len - 1] = 0xD9;
	}
	const uint64_t b0 = t_boff[blockIdx.x], b1 = b0 + t_bits[blockIdx.x];
	const uint32_t h = (uint32_t)(b0 & 7u), n_own = (uint32_t)((b1 >> 3) - (b0 >> 3));
	const uint32_t nwords = (uint32_t)((h + (b1 - b0) + 31) / 32);
	emit_tables_to_lds(T, &tab);
	emit_pack_tile(&tab, s, tl, reinterpret_cast<const int16_t *>(du_base + s.du_off), h, nwords, buf, uoff);
	if (h && threadIdx.x == 0) /* the previous tile's tail completes the first byte */
		buf[0] |= (t_frag[blockIdx.x - 1] >> 8) << (32 - h);
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
	uint8_t *o = out + MIJ_EMIT_HDR + t_out[blockIdx.x] + pos;
	for (uint32_t j = j0; j < j1; ++j) {
		const uint32_t b = lds_byte(buf, j);
		*o++ = (uint8_t)b;
		if (b == 0xFFu)
			*o++ = 0;
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
