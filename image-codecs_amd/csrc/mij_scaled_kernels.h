/*
 * mij_scaled_kernels.h -- reduced-size decode (mij_batch_set_scale, include/mij.h): pictures at 1/2, 1/4 or 1/8 size straight from
 * the coefficients.  Included by mij_runtime.hip.
 *
 * Scale s = 2, 4, 8 and N = 8 / s.  A component with sampling factors (h, v) in a picture with (h_max, v_max) is transformed with an
 * NH = N * h_max / h point row transform and an NV = N * v_max / v point column transform on the low NV x NH coefficients of each block,
 * so every component comes out at the picture's reduced resolution: no upsampling stage exists here.  Output pixel (X, Y) takes sample
 * (Y mod NV, X mod NH) of block (Y div NV, X div NH) of each component; the picture is ceil(W / s) x ceil(H / s).
 *
 * The block transform, exact and integer (tests/scaled_model.py is the numpy restatement):
 *     d[u][v] = (short)(coef * q)                                         u < NV, v < NH -- nothing outside that rectangle is read
 *     t[y][v] = (sum_u K_NV[y][u] * d[u][v] + 512) >> 10                  down the columns
 *     p[y][x] = clamp255((sum_v K_NH[x][v] * t[y][v] + 65536 + (128 << 17)) >> 17)
 * in wrapping 32-bit arithmetic with arithmetic shifts.  K_8 is the reference's STBI__IDCT_1D (idct1d_wide), the shorter transforms
 * are K_n[x][u] = rint(4096 * sqrt(2) * a(u) * cos((2x + 1) u pi / 2n)): DC weight 4096 in every length.  Both passes run in 32 bits for
 * every stream, so the family has no WIDE dimension (MIJ_FLAG_WIDE_IDCT streams take the same kernels).
 *
 * One lane per MCU (the luma-only form: per luma block), 256 consecutive MCUs of a picture per workgroup.  The lane loads only the
 * chunks 0 .. NH-1 of each block (the tile layout keeps column c in chunk c), the DC from the DC array and escape bytes only when
 * the block is flagged, transforms the chroma blocks first (kept as packed bytes), then one luma block row at a time: colour
 * conversion in registers, the pixels into an LDS strip in lane order.  The workgroup then stores the strip: the lanes of one MCU row
 * form one contiguous run of every output row, which leaves as aligned dwords with byte-wise heads and tails (OW * n_out has no
 * alignment to rely on).  Nothing outside the OW x OH x n_out bytes is written.
 */
#pragma once

namespace mij {

enum { SC_Y = 0, SC_444, SC_420, SC_422, SC_LAYOUTS };

/* N-point inverse DCT on s[0 .. N-1] plus BIAS, wrapping; N = 8 is the reference's transform */
template <int N, int BIAS>
__device__ __forceinline__ void sc_idct1d(const int (&s)[8], int (&o)[8])
{
	if constexpr (N == 8) {
		const Idct1D r = idct1d_wide<BIAS>(s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]);
#pragma unroll
		for (int i = 0; i < 8; ++i)
			o[i] = r.o[i];
	} else if constexpr (N == 4) {
		const uint32_t a = (uint32_t)s[0], b = (uint32_t)s[1], c = (uint32_t)s[2], d = (uint32_t)s[3];
		const uint32_t e0 = 4096u * (a + c) + (uint32_t)BIAS, e1 = 4096u * (a - c) + (uint32_t)BIAS;
		const uint32_t o0 = 5352u * b + 2217u * d, o1 = 2217u * b - 5352u * d;
		o[0] = (int)(e0 + o0);
		o[1] = (int)(e1 + o1);
		o[2] = (int)(e1 - o1);
		o[3] = (int)(e0 - o0);
	} else if constexpr (N == 2) {
		const uint32_t a = (uint32_t)s[0], b = (uint32_t)s[1];
		o[0] = (int)(4096u * (a + b) + (uint32_t)BIAS);
		o[1] = (int)(4096u * (a - b) + (uint32_t)BIAS);
	} else {
		o[0] = (int)(4096u * (uint32_t)s[0] + (uint32_t)BIAS);
	}
}

/* The low NV x NH coefficients of block L of one component, de-quantised and transformed: rows[y] holds the NH samples of row y as
 * packed bytes (sample x in byte x & 3 of word x >> 2).  dq = the component's table in in-block position order (wave-uniform). */
template <int NV, int NH, bool B8>
__device__ __forceinline__ void sc_block(const CoefView &cv, uint32_t L, const uint32_t *__restrict__ dq, uint32_t (&rows)[NV][(NH + 3) / 4])
{
	constexpr uint8_t slot[8] = {0, 4, 2, 5, 1, 6, 3, 7}; /* mij_rowslot */
	int t[NV][NH];
	bool esc = false;
	const uint8_t *base;
	if constexpr (B8) {
		base = cv.plane + ((size_t)(L >> 6) << 12) + ((size_t)(L & 63u) << 3);
		if constexpr (NV * NH > 1)
			esc = (base[0] & 1u) != 0; /* the byte in the DC's place holds the block's flags */
	} else {
		base = cv.plane + tile_chunk_off(L, 0);
	}
#pragma unroll
	for (int v = 0; v < NH; ++v) {
		uint32_t c[NV]; /* quantised coefficients of column v, rows 0 .. NV-1, mod 2^16 */
		if constexpr (B8) {
			uint32_t h[2] = {0, 0};
			if constexpr (NV == 1) {
				if (v > 0)
					h[0] = base[v << 9];
			} else {
				const uint2 w = *reinterpret_cast<const uint2 *>(base + (v << 9));
				h[0] = w.x;
				h[1] = w.y;
			}
#pragma unroll
			for (int u = 0; u < NV; ++u)
				c[u] = (uint32_t)(int)(int8_t)(h[slot[u] >> 2] >> (8 * (slot[u] & 3)));
			if (esc) {
				const uint8_t *hp = cv.hi + ((size_t)L << 6) + 8 * v;
#pragma unroll
				for (int u = 0; u < NV; ++u)
					if (u + v > 0)
						c[u] += (uint32_t)((int)(int8_t)hp[slot[u]] * 256);
			}
			if (v == 0)
				c[0] = *reinterpret_cast<const uint16_t *>(cv.dc + 2u * (size_t)L);
		} else {
			if constexpr (NV == 1) {
				c[0] = *reinterpret_cast<const uint16_t *>(base + (v << 10));
			} else {
				const uint4 w = *reinterpret_cast<const uint4 *>(base + (v << 10));
				const uint32_t h[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
				for (int u = 0; u < NV; ++u)
					c[u] = h[slot[u] >> 1] >> (16 * (slot[u] & 1));
			}
		}
		int d[8] = {0, 0, 0, 0, 0, 0, 0, 0}, o[8];
#pragma unroll
		for (int u = 0; u < NV; ++u) {
			const int P = 8 * v + slot[u];
			const uint32_t q = (dq[P >> 1] >> (16 * (P & 1))) & 0xffffu;
			d[u] = (int)(int16_t)(uint16_t)((c[u] & 0xffffu) * q); /* (short)(coef * dequant), codec/jpeg.c:325-365 */
		}
		sc_idct1d<NV, 512>(d, o);
#pragma unroll
		for (int y = 0; y < NV; ++y)
			t[y][v] = o[y] >> 10;
	}
#pragma unroll
	for (int y = 0; y < NV; ++y) {
		int in[8] = {0, 0, 0, 0, 0, 0, 0, 0}, o[8];
#pragma unroll
		for (int v = 0; v < NH; ++v)
			in[v] = t[y][v];
		sc_idct1d<NH, MIJ_PASS2_BIAS>(in, o);
#pragma unroll
		for (int w = 0; w < (NH + 3) / 4; ++w)
			rows[y][w] = 0;
#pragma unroll
		for (int x = 0; x < NH; ++x)
			rows[y][x >> 2] |= (uint32_t)clamp255(opaque(o[x] >> 17)) << (8 * (x & 3)); /* opaque: no compiler-made v_ashr_pk_u8_i32 (mij_kernels.h, sat4) */
		/* the packed words are what stays live: without the vreg() the compiler sees through the packing and keeps every sample in a
		 * register of its own until its pixel is converted (4:2:0 at s = 2: 128 chroma samples, beyond the register file) */
#pragma unroll
		for (int w = 0; w < (NH + 3) / 4; ++w)
			rows[y][w] = vreg(rows[y][w]);
	}
}

__device__ __forceinline__ int sc_byte(uint32_t w, int k) { return (int)((w >> (8 * k)) & 255u); }

/* N pixels of one row into the lane's place of the LDS strip: n_out bytes each (colour: r g b [255]; luma-only: y [255] | y y y [255]) */
template <int N, bool COLOUR>
__device__ __forceinline__ void sc_put_row(uint8_t *__restrict__ dst, int n, const int (&r)[N], const int (&g)[N], const int (&b)[N])
{
	if (n == 4) { /* dst is dword aligned: the lane's place starts at a multiple of 4 * TW bytes */
#pragma unroll
		for (int x = 0; x < N; ++x)
			reinterpret_cast<uint32_t *>(dst)[x] = (uint32_t)r[x] | (uint32_t)g[x] << 8 | (uint32_t)b[x] << 16 | 0xff000000u;
	} else if (n == 3 && N % 4 == 0) { /* 12 bytes per four pixels, dword aligned */
#pragma unroll
		for (int x = 0; x < N; x += 4) {
			uint32_t *w = reinterpret_cast<uint32_t *>(dst + 3 * x);
			w[0] = (uint32_t)r[x] | (uint32_t)g[x] << 8 | (uint32_t)b[x] << 16 | (uint32_t)r[x + 1] << 24;
			w[1] = (uint32_t)g[x + 1] | (uint32_t)b[x + 1] << 8 | (uint32_t)r[x + 2] << 16 | (uint32_t)g[x + 2] << 24;
			w[2] = (uint32_t)b[x + 2] | (uint32_t)r[x + 3] << 8 | (uint32_t)g[x + 3] << 16 | (uint32_t)b[x + 3] << 24;
		}
	} else if (n == 3) {
#pragma unroll
		for (int x = 0; x < N; ++x) {
			dst[3 * x] = (uint8_t)r[x];
			dst[3 * x + 1] = (uint8_t)g[x];
			dst[3 * x + 2] = (uint8_t)b[x];
		}
	} else if (!COLOUR) { /* one or two channels: y | y, 255 (codec/jpeg.c:2373-2430) */
#pragma unroll
		for (int x = 0; x < N; ++x) {
			dst[n * x] = (uint8_t)r[x];
			if (n == 2)
				dst[2 * x + 1] = 255;
		}
	}
}

/* The strip's rows, from LDS to the picture.  The lanes [la, la + nl) of the workgroup hold neighbouring MCUs of one MCU row: row r of the
 * strip is one run of len bytes starting at g0 + r * pitch, found in LDS at lds + r * rowb + la * pxb.  Every thread of the workgroup takes
 * aligned dwords of the runs (LDS is read at whatever byte offset that needs); a dword that crosses an end of its run goes byte by byte. */
__device__ __forceinline__ void sc_store_runs(const uint32_t *__restrict__ lds, uint32_t so0, uint32_t rowb, uint8_t *__restrict__ g0, size_t pitch, uint32_t len, uint32_t nrows)
{
	const uint32_t nd = (len + 6u) >> 2; /* dword slots of a run at the worst misalignment */
	const uint8_t *lb = reinterpret_cast<const uint8_t *>(lds);
	for (uint32_t idx = threadIdx.x; idx < nd * nrows; idx += 256u) {
		const uint32_t r = idx / nd, j = idx - r * nd;
		uint8_t *g = g0 + (size_t)r * pitch;
		const int p = (int)(4u * j) - (int)((uintptr_t)g & 3u); /* first byte of this dword, relative to the run */
		const uint32_t so = so0 + r * rowb;
		if (p >= 0 && (uint32_t)p + 4u <= len) {
			const uint32_t o = so + (uint32_t)p, w0 = lds[o >> 2], w1 = lds[(o >> 2) + 1];
			*reinterpret_cast<uint32_t *>(g + p) = (uint32_t)((((uint64_t)w1 << 32) | w0) >> (8u * (o & 3u)));
		} else {
#pragma unroll
			for (int k = 0; k < 4; ++k)
				if (p + k >= 0 && (uint32_t)(p + k) < len)
					g[p + k] = lb[so + (uint32_t)(p + k)];
		}
	}
}

/* With a table of windows as fifth argument (k_scaled<LAYOUT, S, B8, const DevRoi *>: slots with a region, mij_batch_set_roi) the lane grid
 * is the slot's window -- in MCUs, or luma blocks in the luma-only form -- instead of the picture's grid: the work item's 256 lanes count
 * through it in raster order, and the strips leave from the window's first column.  Without, the kernel compiles to the code it was. */
template <int LAYOUT, int S, bool B8, typename... ROI>
__global__ __launch_bounds__(256) void k_scaled(const DevImage *__restrict__ imgs, const WorkIdct *__restrict__ work, const uint8_t *__restrict__ coef,
																uint8_t *__restrict__ outbase, ROI... rois)
{
	constexpr int N = 8 / S;
	constexpr int HM = (LAYOUT == SC_420 || LAYOUT == SC_422) ? 2 : 1, VM = LAYOUT == SC_420 ? 2 : 1;
	constexpr int TW = N * HM, TH = N * VM; /* the lane's pixel tile; also the chroma transform lengths (NH, NV) */
	constexpr bool COLOUR = LAYOUT != SC_Y, WIN = sizeof...(ROI) != 0;
	__shared__ __attribute__((aligned(16))) uint32_t lds[N * 256 * TW + 4]; /* a strip of N rows, 4 bytes a pixel at the most; + the dword a misaligned read looks into */

	const WorkIdct wk = work[blockIdx.x];
	const DevImage &im = imgs[wk.img];
	/* the lane grid: MCUs, or the luma blocks of whatever layout for the luma-only form */
	const DevRoi rw = roi_of(wk.img, rois...);
	const uint32_t pgx = (uint32_t)(COLOUR ? im.mcu_x : im.comp[0].bw); /* the picture's grid; the window's first unit in it */
	const uint32_t gx = WIN ? rw.w : pgx, gy = WIN ? rw.h : (uint32_t)(COLOUR ? im.mcu_y : im.comp[0].bh), ux0 = WIN ? rw.x0 : 0u, uy0 = WIN ? rw.y0 : 0u;
	const uint32_t nm = gx * gy, m0 = wk.first, cnt = min(256u, nm - m0);
	const uint32_t m = min(m0 + threadIdx.x, nm - 1u); /* lanes past the end redo the last MCU: they load in bounds and their pixels are never stored */
	const uint32_t my = m / gx, mx = m - my * gx;
	const uint32_t n = (uint32_t)im.n_out, OW = ((uint32_t)im.width + S - 1) / S, OH = ((uint32_t)im.height + S - 1) / S;
	const uint32_t pxb = TW * n, rowb = 256u * pxb; /* bytes of a lane's row and of a strip row in LDS */
	uint8_t *const out = outbase + im.out_off;
	uint8_t *const mine = reinterpret_cast<uint8_t *>(lds) + threadIdx.x * pxb;

	uint32_t cb[COLOUR ? TH : 1][(TW + 3) / 4], cr[COLOUR ? TH : 1][(TW + 3) / 4];
	if constexpr (COLOUR) {
		const uint32_t mc = WIN ? (uy0 + my) * pgx + ux0 + mx : m; /* chroma is 1 x 1: its block index is the MCU's */
		sc_block<TH, TW, B8>(coef_view(coef, im.comp[1]), mc, im.dq[1], cb);
		sc_block<TH, TW, B8>(coef_view(coef, im.comp[2]), mc, im.dq[2], cr);
	}
	const CoefView yv = coef_view(coef, im.comp[0]);
	const uint32_t bw0 = (uint32_t)im.comp[0].bw;
	const uint32_t myA = m0 / gx, myB = (m0 + cnt - 1u) / gx; /* the MCU rows this workgroup touches */
#pragma unroll
	for (int dy = 0; dy < VM; ++dy) {
#pragma unroll
		for (int dx = 0; dx < HM; ++dx) {
			uint32_t ys[N][(N + 3) / 4];
			sc_block<N, N, B8>(yv, ((uy0 + my) * VM + dy) * bw0 + (ux0 + mx) * HM + dx, im.dq[0], ys);
#pragma unroll
			for (int y = 0; y < N; ++y) {
				int r[N], g[N], b[N];
#pragma unroll
				for (int x = 0; x < N; ++x) {
					const int lum = sc_byte(ys[y][x >> 2], x & 3);
					if constexpr (COLOUR) {
						const int cx = dx * N + x, cy = dy * N + y;
						ycbcr_to_rgb(lum, sc_byte(cb[cy][cx >> 2], cx & 3), sc_byte(cr[cy][cx >> 2], cx & 3), r[x], g[x], b[x]);
					} else {
						r[x] = g[x] = b[x] = lum;
					}
				}
				sc_put_row<N, COLOUR>(mine + y * rowb + dx * N * n, (int)n, r, g, b);
			}
		}
		__syncthreads();
		for (uint32_t sy = myA; sy <= myB; ++sy) { /* workgroup-uniform */
			const uint32_t a = max(m0, sy * gx), e = min(m0 + cnt, (sy + 1u) * gx); /* MCUs [a, e) of MCU row sy */
			const uint32_t x0 = (ux0 + a - sy * gx) * TW, x1 = min((ux0 + e - sy * gx) * TW, OW), Y0 = (uy0 + sy) * TH + dy * N;
			if (x1 <= x0 || Y0 >= OH)
				continue;
			sc_store_runs(lds, (a - m0) * pxb, rowb, out + ((size_t)Y0 * OW + x0) * n, (size_t)OW * n, (x1 - x0) * n, min((uint32_t)N, OH - Y0));
		}
		if (dy + 1 < VM)
			__syncthreads();
	}
}

} /* namespace mij */
