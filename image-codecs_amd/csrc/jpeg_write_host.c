/*
 * jpeg_write_host.c -- baseline JFIF writer behind stbi_write_jpg / stbi_write_jpg_to_func.
 *
 * Restates the reference encoder (codec/jpeg_write.c:1-388) so that the produced byte stream is
 * identical: same quality mapping and tables (:220-243), same headers (:245-268), the same
 * float colour transform, edge replication and 2x2 chroma mean (:283-325 / :330-352), the same
 * float AAN forward DCT operation order (:24-74, :96-105), the same round-to-nearest quantiser
 * (:107-118) and the same Huffman emission (:120-169, :4-22).  Float results depend on the
 * operation order, so this file must be compiled with -ffp-contract=off and without fast-math.
 *
 * The forward DCT + quantisation of this path (BASELINE config 5) still
 * runs on the host in this round; the GPU kernel for it is the next step behind the same API.
 * The benchmark uses this writer to synthesise its JPEG inputs on the GPU box.
 *
 * The Huffman code tables are derived from the Annex-K BITS/HUFFVAL lists (which the file has
 * to carry anyway for its DHT segment) instead of being spelled out as literal code tables.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>

#include <stdint.h>
#include <emmintrin.h>
#include <xmmintrin.h>

#include "image_api.h"
#include "mij_host.h"

static int g_flip_on_write = 0;
void stbi_flip_vertically_on_write(int flag) { g_flip_on_write = flag; }

/* natural index -> zigzag position (codec/jpeg_write.c:1-2) */
static const unsigned char k_zigzag_of[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
															 41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
															 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

/* Annex K.3 tables: BITS (index 0 unused) and HUFFVAL */
static const unsigned char k_dc_lum_bits[17] = {0, 0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
static const unsigned char k_dc_vals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const unsigned char k_dc_chr_bits[17] = {0, 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
static const unsigned char k_ac_lum_bits[17] = {0, 0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
static const unsigned char k_ac_lum_vals[162] = {
	0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
	0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
	0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
	0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
	0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
	0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
	0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
	0xfa};
static const unsigned char k_ac_chr_bits[17] = {0, 0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
static const unsigned char k_ac_chr_vals[162] = {
	0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
	0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
	0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
	0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
	0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
	0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
	0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
	0xfa};

/* base quantisation tables, natural order (codec/jpeg_write.c:204-207) */
static const int k_qt_lum[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
											69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
											81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
static const int k_qt_chr[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
											99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

typedef struct {
	unsigned short code[256], len[256];
} enc_table;

/* canonical code assignment of Annex C: gives the reference's literal YDC_HT/UVDC_HT/YAC_HT/UVAC_HT */
static void make_enc_table(enc_table *t, const unsigned char *bits, const unsigned char *vals)
{
	int l, i, k = 0;
	unsigned code = 0;
	memset(t, 0, sizeof(*t));
	for (l = 1; l <= 16; ++l) {
		for (i = 0; i < bits[l]; ++i, ++k) {
			t->code[vals[k]] = (unsigned short)code++;
			t->len[vals[k]] = (unsigned short)l;
		}
		code <<= 1;
	}
}

/* Output side.  The reference pushes every byte through the callback one at a time from a 24-bit bit buffer
 * (codec/jpeg_write.c:4-22); the byte stream is a function of the symbols alone, so here the bits gather in a 64-bit
 * accumulator and leave four bytes at a time -- byte stuffing (0xFF -> 0xFF 0x00) only when one of the four is 0xFF --
 * into a buffer handed to the callback in chunks of up to 4 KiB.  1080p: 7 ms -> 2.6 ms per picture. */
typedef struct {
	stbi_write_func *func;
	void *context;
	unsigned char buf[4096 + 16];
	int used;
	uint64_t acc; /* the low `nacc` bits are pending output, oldest bit highest */
	int nacc;
} jw_sink;

static void sink_flush(jw_sink *s)
{
	if (s->used) {
		s->func(s->context, s->buf, s->used);
		s->used = 0;
	}
}
static inline void sink_byte(jw_sink *s, unsigned char c)
{
	if (s->used >= 4096)
		sink_flush(s);
	s->buf[s->used++] = c;
}
static void sink_bytes(jw_sink *s, const void *p, int n)
{
	const unsigned char *b = (const unsigned char *)p;
	int i;
	for (i = 0; i < n; ++i)
		sink_byte(s, b[i]);
}

/* codec/jpeg_write.c:4-22: len <= 27 bits (a code of at most 16 plus at most 11 magnitude bits) */
static inline void put_bits(jw_sink *s, unsigned code, int len)
{
	s->acc = (s->acc << len) | (uint64_t)code;
	s->nacc += len;
	if (s->nacc >= 32) {
		const uint32_t w = (uint32_t)(s->acc >> (s->nacc - 32));
		s->nacc -= 32;
		if (s->used > 4096 - 8)
			sink_flush(s);
		/* a byte of w is 0xFF <=> the same byte of ~w is zero (the classic has-zero-byte test) */
		if ((((~w) - 0x01010101u) & w & 0x80808080u) == 0) {
			unsigned char *o = s->buf + s->used;
			o[0] = (unsigned char)(w >> 24);
			o[1] = (unsigned char)(w >> 16);
			o[2] = (unsigned char)(w >> 8);
			o[3] = (unsigned char)w;
			s->used += 4;
		} else {
			int k;
			for (k = 24; k >= 0; k -= 8) {
				const unsigned char c = (unsigned char)(w >> k);
				s->buf[s->used++] = c;
				if (c == 255)
					s->buf[s->used++] = 0;
			}
		}
	}
}

/* the whole bytes still pending (the reference emits a byte as soon as it has eight bits; what is left below a byte after the
 * final fill bits is dropped there too, codec/jpeg_write.c:358-360) */
static void put_bits_finish(jw_sink *s)
{
	while (s->nacc >= 8) {
		const unsigned char c = (unsigned char)(s->acc >> (s->nacc - 8));
		s->nacc -= 8;
		sink_byte(s, c);
		if (c == 255)
			sink_byte(s, 0);
	}
}

/* magnitude category and the bits that follow it (codec/jpeg_write.c:76-86); val != 0 */
static inline void magnitude_bits(int val, unsigned *bits, int *nbits)
{
	const unsigned a = (unsigned)(val < 0 ? -val : val);
	const int v = val < 0 ? val - 1 : val, n = 32 - __builtin_clz(a);
	*nbits = n;
	*bits = (unsigned)v & ((1u << n) - 1u);
}

/* one 8-point AAN pass over p[0], p[s], ... p[7s]; operation order of codec/jpeg_write.c:24-74 */
static inline void fdct8(float *p, int s)
{
	float d0 = p[0], d1 = p[s], d2 = p[2 * s], d3 = p[3 * s], d4 = p[4 * s], d5 = p[5 * s], d6 = p[6 * s], d7 = p[7 * s];
	float a0 = d0 + d7, a7 = d0 - d7;
	float a1 = d1 + d6, a6 = d1 - d6;
	float a2 = d2 + d5, a5 = d2 - d5;
	float a3 = d3 + d4, a4 = d3 - d4;
	/* even part */
	float b0 = a0 + a3, b3 = a0 - a3;
	float b1 = a1 + a2, b2 = a1 - a2;
	float z1, z2, z3, z4, z5, z11, z13;
	float o0 = b0 + b1, o4 = b0 - b1;
	float o2, o6;
	z1 = (b2 + b3) * 0.707106781f;
	o2 = b3 + z1;
	o6 = b3 - z1;
	/* odd part */
	b0 = a4 + a5;
	b1 = a5 + a6;
	b2 = a6 + a7;
	z5 = (b0 - b2) * 0.382683433f;
	z2 = b0 * 0.541196100f + z5;
	z4 = b2 * 1.306562965f + z5;
	z3 = b1 * 0.707106781f;
	z11 = a7 + z3;
	z13 = a7 - z3;
	p[5 * s] = z13 + z2;
	p[3 * s] = z13 - z2;
	p[s] = z11 + z4;
	p[7 * s] = z11 - z4;
	p[0] = o0;
	p[2 * s] = o2;
	p[4 * s] = o4;
	p[6 * s] = o6;
}

/* The same pass on four independent 1-D transforms at once (one per SSE lane): every lane performs exactly the operations of
 * fdct8 in exactly its order -- mulps / addps / subps are IEEE single operations, nothing is contracted (-ffp-contract=off) --
 * so the results are the scalar code's bit for bit. */
static inline void fdct8_ps(__m128 *d)
{
	const __m128 c707 = _mm_set1_ps(0.707106781f), c382 = _mm_set1_ps(0.382683433f), c541 = _mm_set1_ps(0.541196100f), c1306 = _mm_set1_ps(1.306562965f);
	const __m128 a0 = _mm_add_ps(d[0], d[7]), a7 = _mm_sub_ps(d[0], d[7]), a1 = _mm_add_ps(d[1], d[6]), a6 = _mm_sub_ps(d[1], d[6]);
	const __m128 a2 = _mm_add_ps(d[2], d[5]), a5 = _mm_sub_ps(d[2], d[5]), a3 = _mm_add_ps(d[3], d[4]), a4 = _mm_sub_ps(d[3], d[4]);
	__m128 b0 = _mm_add_ps(a0, a3), b3 = _mm_sub_ps(a0, a3), b1 = _mm_add_ps(a1, a2), b2 = _mm_sub_ps(a1, a2);
	const __m128 o0 = _mm_add_ps(b0, b1), o4 = _mm_sub_ps(b0, b1);
	const __m128 z1 = _mm_mul_ps(_mm_add_ps(b2, b3), c707);
	const __m128 o2 = _mm_add_ps(b3, z1), o6 = _mm_sub_ps(b3, z1);
	__m128 z2, z3, z4, z5, z11, z13;
	b0 = _mm_add_ps(a4, a5);
	b1 = _mm_add_ps(a5, a6);
	b2 = _mm_add_ps(a6, a7);
	z5 = _mm_mul_ps(_mm_sub_ps(b0, b2), c382);
	z2 = _mm_add_ps(_mm_mul_ps(b0, c541), z5);
	z4 = _mm_add_ps(_mm_mul_ps(b2, c1306), z5);
	z3 = _mm_mul_ps(b1, c707);
	z11 = _mm_add_ps(a7, z3);
	z13 = _mm_sub_ps(a7, z3);
	d[5] = _mm_add_ps(z13, z2);
	d[3] = _mm_sub_ps(z13, z2);
	d[1] = _mm_add_ps(z11, z4);
	d[7] = _mm_sub_ps(z11, z4);
	d[0] = o0;
	d[2] = o2;
	d[4] = o4;
	d[6] = o6;
}

/* forward DCT + quantise one data unit into zigzag order (codec/jpeg_write.c:96-118): rows, then columns, then
 * "(int)(v < 0 ? v - 0.5f : v + 0.5f)" with v = coefficient * fdtbl.  Row pass: the block is transposed so that the eight row
 * transforms sit in SSE lanes, transformed, transposed back; the column pass has its transforms in lanes as the block lies. */
static void transform_du(float *cdu, int stride, const float *fdtbl, int16_t *du)
{
	__m128 lo[8], hi[8], t[8];
	int y, j;
	for (y = 0; y < 8; ++y) {
		lo[y] = _mm_loadu_ps(cdu + y * stride);
		hi[y] = _mm_loadu_ps(cdu + y * stride + 4);
	}
	/* rows 0..3 and 4..7 as lanes: t[k] = (column k of rows 0..3), u[k] = (column k of rows 4..7) */
	{
		__m128 u[8];
		__m128 r0 = lo[0], r1 = lo[1], r2 = lo[2], r3 = lo[3];
		_MM_TRANSPOSE4_PS(r0, r1, r2, r3);
		t[0] = r0, t[1] = r1, t[2] = r2, t[3] = r3;
		r0 = hi[0], r1 = hi[1], r2 = hi[2], r3 = hi[3];
		_MM_TRANSPOSE4_PS(r0, r1, r2, r3);
		t[4] = r0, t[5] = r1, t[6] = r2, t[7] = r3;
		r0 = lo[4], r1 = lo[5], r2 = lo[6], r3 = lo[7];
		_MM_TRANSPOSE4_PS(r0, r1, r2, r3);
		u[0] = r0, u[1] = r1, u[2] = r2, u[3] = r3;
		r0 = hi[4], r1 = hi[5], r2 = hi[6], r3 = hi[7];
		_MM_TRANSPOSE4_PS(r0, r1, r2, r3);
		u[4] = r0, u[5] = r1, u[6] = r2, u[7] = r3;
		fdct8_ps(t);
		fdct8_ps(u);
		/* back: row y = (t[0..7] lane y) for y < 4, (u[0..7] lane y - 4) otherwise */
		r0 = t[0], r1 = t[1], r2 = t[2], r3 = t[3];
		_MM_TRANSPOSE4_PS(r0, r1, r2, r3);
		lo[0] = r0, lo[1] = r1, lo[2] = r2, lo[3] = r3;
		r0 = t[4], r1 = t[5], r2 = t[6], r3 = t[7];
		_MM_TRANSPOSE4_PS(r0, r1, r2, r3);
		hi[0] = r0, hi[1] = r1, hi[2] = r2, hi[3] = r3;
		r0 = u[0], r1 = u[1], r2 = u[2], r3 = u[3];
		_MM_TRANSPOSE4_PS(r0, r1, r2, r3);
		lo[4] = r0, lo[5] = r1, lo[6] = r2, lo[7] = r3;
		r0 = u[4], r1 = u[5], r2 = u[6], r3 = u[7];
		_MM_TRANSPOSE4_PS(r0, r1, r2, r3);
		hi[4] = r0, hi[5] = r1, hi[6] = r2, hi[7] = r3;
	}
	fdct8_ps(lo); /* columns 0..3 */
	fdct8_ps(hi); /* columns 4..7 */
	for (y = 0, j = 0; y < 8; ++y, j += 8) {
		const __m128 half = _mm_set1_ps(0.5f), zero = _mm_setzero_ps();
		const __m128 va = _mm_mul_ps(lo[y], _mm_loadu_ps(fdtbl + j)), vb = _mm_mul_ps(hi[y], _mm_loadu_ps(fdtbl + j + 4));
		/* v < 0 ? v - 0.5f : v + 0.5f, then the C cast's truncation */
		const __m128 ma = _mm_cmplt_ps(va, zero), mb = _mm_cmplt_ps(vb, zero);
		const __m128 ra = _mm_or_ps(_mm_and_ps(ma, _mm_sub_ps(va, half)), _mm_andnot_ps(ma, _mm_add_ps(va, half)));
		const __m128 rb = _mm_or_ps(_mm_and_ps(mb, _mm_sub_ps(vb, half)), _mm_andnot_ps(mb, _mm_add_ps(vb, half)));
		int32_t q[8];
		int x;
		_mm_storeu_si128((__m128i *)q, _mm_cvttps_epi32(ra));
		_mm_storeu_si128((__m128i *)(q + 4), _mm_cvttps_epi32(rb));
		for (x = 0; x < 8; ++x)
			du[k_zigzag_of[j + x]] = (int16_t)q[x];
	}
}

/* Huffman-code one quantised data unit (codec/jpeg_write.c:120-169); returns its DC.  The reference scans the unit for its last
 * non-zero coefficient and then for every run of zeros; the same symbols come out of walking the set bits of the unit's
 * non-zero mask (sixteen int16 per SSE2 compare), a code and its magnitude bits leaving in one put_bits. */
static int emit_du(jw_sink *s, const int16_t *du, int dc_pred, const enc_table *hdc, const enc_table *hac)
{
	const int diff = du[0] - dc_pred;
	unsigned bits;
	int nbits, prev = 0, k;
	uint64_t nz = 0;
	const __m128i zero = _mm_setzero_si128();
	if (diff == 0) {
		put_bits(s, hdc->code[0], hdc->len[0]);
	} else {
		magnitude_bits(diff, &bits, &nbits);
		put_bits(s, ((unsigned)hdc->code[nbits] << nbits) | bits, hdc->len[nbits] + nbits);
	}
	for (k = 0; k < 4; ++k) {
		const __m128i a = _mm_loadu_si128((const __m128i *)(du + 16 * k)), b = _mm_loadu_si128((const __m128i *)(du + 16 * k + 8));
		const unsigned m = (unsigned)_mm_movemask_epi8(_mm_packs_epi16(_mm_cmpeq_epi16(a, zero), _mm_cmpeq_epi16(b, zero))); /* bit i: coefficient is zero */
		nz |= (uint64_t)(~m & 0xffffu) << (16 * k);
	}
	nz &= ~(uint64_t)1;
	if (!nz) {
		put_bits(s, hac->code[0x00], hac->len[0x00]);
		return du[0];
	}
	while (nz) {
		const int i = __builtin_ctzll(nz);
		int run = i - prev - 1;
		prev = i;
		nz &= nz - 1;
		for (; run >= 16; run -= 16)
			put_bits(s, hac->code[0xF0], hac->len[0xF0]);
		magnitude_bits(du[i], &bits, &nbits);
		put_bits(s, ((unsigned)hac->code[(run << 4) + nbits] << nbits) | bits, hac->len[(run << 4) + nbits] + nbits);
	}
	if (prev != 63)
		put_bits(s, hac->code[0x00], hac->len[0x00]);
	return du[0];
}

/*
 * The writer in three separable steps (so that step 2 can run on the GPU, mij_enc_* in mij.h):
 *   1. mjw_plan_init      quality mapping, quantisation + scaled-reciprocal tables (codec/jpeg_write.c:220-243)
 *   2. mjw_transform_host colour transform, edge replication, 2x2 chroma mean, fDCT, quantiser for every
 *                         data unit (:283-352 minus the Huffman calls): DU blocks, MCU order, zigzag order
 *   3. mjw_emit           headers (:245-268), Huffman emission (:120-169), padding and EOI (:358-363)
 */

/* the two tables at a quality in 1..100, zigzag order: mjw_plan_init's, and mjw_quality_tables' for the requantising transcode */
static void quality_tables(int quality, unsigned char *ytab, unsigned char *ctab)
{
	int i;
	quality = quality < 50 ? 5000 / quality : 200 - quality * 2;
	for (i = 0; i < 64; ++i) {
		int yq = (k_qt_lum[i] * quality + 50) / 100;
		int cq = (k_qt_chr[i] * quality + 50) / 100;
		ytab[k_zigzag_of[i]] = (unsigned char)(yq < 1 ? 1 : (yq > 255 ? 255 : yq));
		ctab[k_zigzag_of[i]] = (unsigned char)(cq < 1 ? 1 : (cq > 255 ? 255 : cq));
	}
}

int mjw_quality_tables(int quality, unsigned char luma[64], unsigned char chroma[64])
{
	if (!luma || !chroma || quality < 1 || quality > 100)
		return 0;
	quality_tables(quality, luma, chroma);
	return 1;
}

int mjw_plan_init(mjw_plan *p, int width, int height, int comp, int quality)
{
	static const float aasf[8] = {1.0f * 2.828427125f,         1.387039845f * 2.828427125f, 1.306562965f * 2.828427125f, 1.175875602f * 2.828427125f,
											1.0f * 2.828427125f,         0.785694958f * 2.828427125f, 0.541196100f * 2.828427125f, 0.275899379f * 2.828427125f};
	int row, col, k, mcu;
	if (!p || !width || !height || comp > 4 || comp < 1 || width < 0 || height < 0)
		return 0;
	quality = quality ? quality : 90;
	p->subsample = quality <= 90 ? 1 : 0;
	quality_tables(quality < 1 ? 1 : (quality > 100 ? 100 : quality), p->ytab, p->ctab);
	for (row = 0, k = 0; row < 8; ++row)
		for (col = 0; col < 8; ++col, ++k) {
			p->fdtbl_y[k] = 1 / (p->ytab[k_zigzag_of[k]] * aasf[row] * aasf[col]);
			p->fdtbl_c[k] = 1 / (p->ctab[k_zigzag_of[k]] * aasf[row] * aasf[col]);
		}
	p->width = width;
	p->height = height;
	p->comp = comp;
	mcu = p->subsample ? 16 : 8;
	p->mcu_x = (width + mcu - 1) / mcu;
	p->mcu_y = (height + mcu - 1) / mcu;
	p->du_per_mcu = p->subsample ? 6 : 3;
	return 1;
}

size_t mjw_plan_du_count(const mjw_plan *p) { return (size_t)p->mcu_x * (size_t)p->mcu_y * (size_t)p->du_per_mcu; }

void mjw_transform_host(const mjw_plan *p, const void *data, int flip, int16_t *du)
{
	const int width = p->width, height = p->height, comp = p->comp;
	const int og = comp > 2 ? 1 : 0, ob = comp > 2 ? 2 : 0; /* comp 1/2: grey replicated */
	const unsigned char *px = (const unsigned char *)data;
	const int mcu = p->subsample ? 16 : 8;
	int x, y, row, col, pos;
	float Y[256], U[256], V[256], R[256], G[256], B[256];
	for (y = 0; y < height; y += mcu)
		for (x = 0; x < width; x += mcu) {
			const int npx = mcu * mcu;
			for (row = y, pos = 0; row < y + mcu; ++row) {
				int crow = row < height ? row : height - 1; /* replicate the last row / column */
				int base = (flip ? (height - 1 - crow) : crow) * width * comp;
				for (col = x; col < x + mcu; ++col, ++pos) {
					int q = base + (col < width ? col : width - 1) * comp;
					R[pos] = px[q], G[pos] = px[q + og], B[pos] = px[q + ob];
				}
			}
			/* codec/jpeg_write.c:298-300, four pixels per step; the association of the scalar expressions:
			 *   Y = ((0.299 r + 0.587 g) + 0.114 b) - 128    U = ((-0.16874 r) - 0.33126 g) + 0.5 b    V = ((0.5 r) - 0.41869 g) - 0.08131 b */
			for (pos = 0; pos < npx; pos += 4) {
				const __m128 r = _mm_loadu_ps(R + pos), g = _mm_loadu_ps(G + pos), b = _mm_loadu_ps(B + pos);
				_mm_storeu_ps(Y + pos, _mm_sub_ps(_mm_add_ps(_mm_add_ps(_mm_mul_ps(_mm_set1_ps(+0.29900f), r), _mm_mul_ps(_mm_set1_ps(0.58700f), g)),
																			  _mm_mul_ps(_mm_set1_ps(0.11400f), b)), _mm_set1_ps(128.0f)));
				_mm_storeu_ps(U + pos, _mm_add_ps(_mm_sub_ps(_mm_mul_ps(_mm_set1_ps(-0.16874f), r), _mm_mul_ps(_mm_set1_ps(0.33126f), g)),
															 _mm_mul_ps(_mm_set1_ps(0.50000f), b)));
				_mm_storeu_ps(V + pos, _mm_sub_ps(_mm_sub_ps(_mm_mul_ps(_mm_set1_ps(+0.50000f), r), _mm_mul_ps(_mm_set1_ps(0.41869f), g)),
															 _mm_mul_ps(_mm_set1_ps(0.08131f), b)));
			}
			if (p->subsample) {
				float su[64], sv[64];
				int yy, xx;
				transform_du(Y + 0, 16, p->fdtbl_y, du);
				transform_du(Y + 8, 16, p->fdtbl_y, du + 64);
				transform_du(Y + 128, 16, p->fdtbl_y, du + 128);
				transform_du(Y + 136, 16, p->fdtbl_y, du + 192);
				for (yy = 0, pos = 0; yy < 8; ++yy)
					for (xx = 0; xx < 8; ++xx, ++pos) {
						int j = yy * 32 + xx * 2;
						su[pos] = (U[j + 0] + U[j + 1] + U[j + 16] + U[j + 17]) * 0.25f;
						sv[pos] = (V[j + 0] + V[j + 1] + V[j + 16] + V[j + 17]) * 0.25f;
					}
				transform_du(su, 8, p->fdtbl_c, du + 256);
				transform_du(sv, 8, p->fdtbl_c, du + 320);
				du += 384;
			} else {
				transform_du(Y, 8, p->fdtbl_y, du);
				transform_du(U, 8, p->fdtbl_c, du + 64);
				transform_du(V, 8, p->fdtbl_c, du + 128);
				du += 192;
			}
		}
}

/* The headers in front of the entropy-coded segment (codec/jpeg_write.c:245-268): SOI, APP0, DQT, SOF0, DHT, SOS. */
size_t mjw_header(const mjw_plan *p, unsigned char *out)
{
	static const unsigned char soi_app0_dqt[] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 0x10, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0, 0xFF, 0xDB, 0, 0x84, 0};
	static const unsigned char sos[] = {0xFF, 0xDA, 0, 0xC, 3, 1, 0, 2, 0x11, 3, 0x11, 0, 0x3F, 0};
	unsigned char sof_dht[24] = {0xFF, 0xC0, 0, 0x11, 8, 0, 0, 0, 0, 3, 1, 0, 0, 2, 0x11, 1, 3, 0x11, 1, 0xFF, 0xC4, 0x01, 0xA2, 0};
	unsigned char *o = out;
	sof_dht[5] = (unsigned char)(p->height >> 8);
	sof_dht[6] = (unsigned char)(p->height & 0xff);
	sof_dht[7] = (unsigned char)(p->width >> 8);
	sof_dht[8] = (unsigned char)(p->width & 0xff);
	sof_dht[11] = (unsigned char)(p->subsample ? 0x22 : 0x11);
#define PUT(src, n) (memcpy(o, (src), (n)), o += (n))
	PUT(soi_app0_dqt, sizeof(soi_app0_dqt));
	PUT(p->ytab, 64);
	*o++ = 1;
	PUT(p->ctab, 64);
	PUT(sof_dht, sizeof(sof_dht));
	PUT(k_dc_lum_bits + 1, 16);
	PUT(k_dc_vals, 12);
	*o++ = 0x10;
	PUT(k_ac_lum_bits + 1, 16);
	PUT(k_ac_lum_vals, 162);
	*o++ = 1;
	PUT(k_dc_chr_bits + 1, 16);
	PUT(k_dc_vals, 12);
	*o++ = 0x11;
	PUT(k_ac_chr_bits + 1, 16);
	PUT(k_ac_chr_vals, 162);
	PUT(sos, sizeof(sos));
#undef PUT
	return (size_t)(o - out);
}

void mjw_huff_tables(uint16_t code[4][256], uint8_t len[4][256])
{
	enc_table t[4];
	int k, i;
	make_enc_table(&t[0], k_dc_lum_bits, k_dc_vals);
	make_enc_table(&t[1], k_dc_chr_bits, k_dc_vals);
	make_enc_table(&t[2], k_ac_lum_bits, k_ac_lum_vals);
	make_enc_table(&t[3], k_ac_chr_bits, k_ac_chr_vals);
	for (k = 0; k < 4; ++k)
		for (i = 0; i < 256; ++i) {
			code[k][i] = t[k].code[i];
			len[k][i] = (uint8_t)t[k].len[i];
		}
}

/* headers (hdr_len bytes), the entropy-coded segment under the four tables, fill and EOI */
/* ri > 0: a restart interval of ri MCUs (include/mij_host.h, RESTART INTERVALS): the fill of the scan's end after every ri MCUs that are not the
 * scan's last, the marker RSTk behind it, the DC predictors back at 0 */
static int emit_units_with(size_t nm, int ny, int ncomp, size_t ri, const int16_t *du, mjw_write_func *func, void *context, const enc_table *ydc,
									const enc_table *yac, const enc_table *cdc, const enc_table *cac, const unsigned char *hdr, size_t hdr_len)
{
	jw_sink *s = (jw_sink *)calloc(1, sizeof(*s));
	if (!s)
		return 0;
	s->func = func;
	s->context = context;
	sink_bytes(s, hdr, (int)hdr_len); /* headers (codec/jpeg_write.c:245-268) */
	{
		int dcy = 0, dcu = 0, dcv = 0;
		size_t m, left = ri;
		unsigned rst = 0;
		int k;
		s->acc = 0;
		s->nacc = 0;
		for (m = 0; m < nm; ++m) { /* an MCU: its ny luma units, then Cb and Cr where the picture has them */
			for (k = 0; k < ny; ++k, du += 64)
				dcy = emit_du(s, du, dcy, ydc, yac);
			if (ncomp == 3) {
				dcu = emit_du(s, du, dcu, cdc, cac);
				dcv = emit_du(s, du + 64, dcv, cdc, cac);
				du += 128;
			}
			if (ri && --left == 0 && m + 1 < nm) { /* an interval ends as the scan does; what is left below a byte is dropped */
				put_bits(s, 0x7F, 7);
				put_bits_finish(s);
				s->acc = 0;
				s->nacc = 0;
				sink_byte(s, 0xFF);
				sink_byte(s, (unsigned char)(0xD0 + (rst++ & 7u)));
				dcy = dcu = dcv = 0;
				left = ri;
			}
		}
		put_bits(s, 0x7F, 7); /* pad to a byte boundary with ones */
		put_bits_finish(s);
	}
	sink_byte(s, 0xFF);
	sink_byte(s, 0xD9);
	sink_flush(s);
	free(s);
	return 1;
}
static int emit_with(const mjw_plan *p, const int16_t *du, mjw_write_func *func, void *context, const enc_table *ydc, const enc_table *yac,
							const enc_table *cdc, const enc_table *cac, const unsigned char *hdr, size_t hdr_len)
{
	return emit_units_with((size_t)p->mcu_x * (size_t)p->mcu_y, p->subsample ? 4 : 1, 3, 0, du, func, context, ydc, yac, cdc, cac, hdr, hdr_len);
}

int mjw_emit(const mjw_plan *p, const int16_t *du, mjw_write_func *func, void *context)
{
	enc_table ydc, yac, cdc, cac;
	unsigned char hdr[MJW_HEADER_BYTES];
	if (!func || !du)
		return 0;
	make_enc_table(&ydc, k_dc_lum_bits, k_dc_vals);
	make_enc_table(&cdc, k_dc_chr_bits, k_dc_vals);
	make_enc_table(&yac, k_ac_lum_bits, k_ac_lum_vals);
	make_enc_table(&cac, k_ac_chr_bits, k_ac_chr_vals);
	return emit_with(p, du, func, context, &ydc, &yac, &cdc, &cac, hdr, mjw_header(p, hdr));
}

/* ---- optimised Huffman tables (include/mij_host.h): the symbols mjw_emit emits, counted; ITU-T T.81 K.2 on the counts */

/* one unit's symbols into its DC and AC histograms: emit_du's walk with counts in place of codes */
static int count_du(const int16_t *du, int dc_pred, uint32_t *fdc, uint32_t *fac)
{
	const int diff = du[0] - dc_pred;
	unsigned bits;
	int nbits = 0, prev = 0, i;
	if (diff)
		magnitude_bits(diff, &bits, &nbits);
	++fdc[nbits];
	for (i = 1; i < 64; ++i)
		if (du[i]) {
			const int run = i - prev - 1;
			prev = i;
			fac[0xF0] += (uint32_t)(run >> 4);
			magnitude_bits(du[i], &bits, &nbits);
			++fac[(((run & 15) << 4) + nbits) & 255];
		}
	if (prev != 63)
		++fac[0x00];
	return du[0];
}

static void histogram_units(size_t nm, int ny, int ncomp, size_t ri, const int16_t *du, uint32_t freq[4][256])
{
	int dcy = 0, dcu = 0, dcv = 0;
	size_t m, left = ri;
	memset(freq, 0, sizeof(uint32_t) * 4 * 256);
	for (m = 0; m < nm; ++m) {
		int k;
		for (k = 0; k < ny; ++k, du += 64)
			dcy = count_du(du, dcy, freq[0], freq[2]);
		if (ncomp == 3) {
			dcu = count_du(du, dcu, freq[1], freq[3]);
			dcv = count_du(du + 64, dcv, freq[1], freq[3]);
			du += 128;
		}
		if (ri && --left == 0) { /* the next MCU starts an interval: its DC categories are those of differences against 0 */
			dcy = dcu = dcv = 0;
			left = ri;
		}
	}
}

int mjw_histogram(const mjw_plan *p, const int16_t *du, uint32_t freq[4][256])
{
	if (!p || !du || !freq || mjw_plan_du_count(p) > (size_t)(UINT32_MAX / 64))
		return 0;
	histogram_units((size_t)p->mcu_x * (size_t)p->mcu_y, p->subsample ? 4 : 1, 3, 0, du, freq);
	return 1;
}

int mjw_optimal_table(const uint32_t freq_in[256], uint8_t bits_out[16], uint8_t vals[256], int *nvals)
{
	uint64_t freq[257];
	int codesize[257], others[257], bits[33], i, j, n = 0;
	if (!freq_in || !bits_out || !vals || !nvals)
		return 0;
	for (i = 0; i < 256; ++i)
		freq[i] = freq_in[i];
	freq[256] = 1; /* the pseudo-symbol that keeps the all-ones code free */
	for (i = 0; i < 257; ++i) {
		codesize[i] = 0;
		others[i] = -1;
	}
	for (;;) {
		int c1 = -1, c2 = -1;
		uint64_t v = UINT64_MAX;
		for (i = 0; i <= 256; ++i)
			if (freq[i] && freq[i] <= v) {
				v = freq[i];
				c1 = i;
			}
		v = UINT64_MAX;
		for (i = 0; i <= 256; ++i)
			if (freq[i] && freq[i] <= v && i != c1) {
				v = freq[i];
				c2 = i;
			}
		if (c2 < 0)
			break;
		freq[c1] += freq[c2];
		freq[c2] = 0;
		for (++codesize[c1]; others[c1] >= 0; ++codesize[c1])
			c1 = others[c1];
		others[c1] = c2;
		for (++codesize[c2]; others[c2] >= 0; ++codesize[c2])
			c2 = others[c2];
	}
	memset(bits, 0, sizeof(bits));
	for (i = 0; i <= 256; ++i)
		if (codesize[i]) {
			if (codesize[i] > 32)
				return 0;
			++bits[codesize[i]];
		}
	for (i = 32; i > 16; --i)
		while (bits[i] > 0) {
			for (j = i - 2; bits[j] == 0; --j)
				;
			bits[i] -= 2;
			++bits[i - 1];
			bits[j + 1] += 2;
			--bits[j];
		}
	for (i = 16; i > 0 && bits[i] == 0; --i)
		;
	if (i > 0)
		--bits[i]; /* the pseudo-symbol's code */
	for (i = 1; i <= 16; ++i)
		bits_out[i - 1] = (uint8_t)bits[i];
	for (i = 1; i <= 32; ++i)
		for (j = 0; j < 256; ++j)
			if (codesize[j] == i)
				vals[n++] = (uint8_t)j;
	*nvals = n;
	return 1;
}

size_t mjw_header_optimized(const mjw_plan *p, const uint8_t bits[4][16], const uint8_t vals[4][256], unsigned char *out)
{
	static const unsigned char sos[] = {0xFF, 0xDA, 0, 0xC, 3, 1, 0, 2, 0x11, 3, 0x11, 0, 0x3F, 0};
	static const unsigned char ids[4] = {0x00, 0x10, 0x01, 0x11};
	static const int order[4] = {0, 2, 1, 3}; /* mjw_header's: luma DC, luma AC, chroma DC, chroma AC */
	unsigned char plain[MJW_HEADER_BYTES], *o = out + 177;
	int k, i, n;
	mjw_header(p, plain);
	memcpy(out, plain, 177); /* up to and including the DHT length */
	for (k = 0; k < 4; ++k) {
		const int t = order[k];
		for (i = 0, n = 0; i < 16; ++i)
			n += bits[t][i];
		*o++ = ids[k];
		memcpy(o, bits[t], 16);
		memcpy(o + 16, vals[t], (size_t)n);
		o += 16 + n;
	}
	n = (int)(o - (out + 175));
	out[175] = (unsigned char)(n >> 8);
	out[176] = (unsigned char)(n & 0xff);
	memcpy(o, sos, sizeof(sos));
	return (size_t)(o - out) + sizeof(sos);
}

int mjw_optimized_tables(const mjw_plan *p, const int16_t *du, uint8_t bits[4][16], uint8_t vals[4][256])
{
	uint32_t freq[4][256];
	int t, n;
	if (!mjw_histogram(p, du, freq))
		return 0;
	for (t = 0; t < 4; ++t) {
		memset(vals[t], 0, 256);
		if (!mjw_optimal_table(freq[t], bits[t], vals[t], &n))
			return 0;
	}
	return 1;
}

int mjw_emit_optimized(const mjw_plan *p, const int16_t *du, mjw_write_func *func, void *context)
{
	uint8_t bits[4][16], vals[4][256];
	unsigned char b17[17], hdr[MJW_HEADER_BYTES];
	enc_table t[4];
	int k;
	if (!func || !du || !p)
		return 0;
	if (!mjw_optimized_tables(p, du, bits, vals))
		return mjw_emit(p, du, func, context); /* a code longer than 32 bits before limiting: the plain tables */
	for (k = 0; k < 4; ++k) {
		b17[0] = 0;
		memcpy(b17 + 1, bits[k], 16);
		make_enc_table(&t[k], b17, vals[k]);
	}
	return emit_with(p, du, func, context, &t[0], &t[2], &t[1], &t[3], hdr, mjw_header_optimized(p, bits, vals, hdr));
}

/* ---- lossless transcode (include/mij_host.h, mjw_tplan): the same emission over the five MCU shapes a transcodable source has, with the
 * source's own quantisation tables in the header */

static int tplan_ny(const mjw_tplan *t) { return t->ncomp == 1 ? 1 : t->lh * t->lv; }
size_t mjw_tplan_du_count(const mjw_tplan *t) { return t ? mjw_plan_du_count(&t->plan) : 0; }

/* SOI, APP0, DQT and the frame header under marker `sof` (0xC0 baseline, 0xC2 progressive); a grey picture carries one quantisation table
 * and one component */
static size_t theader_frame(const mjw_tplan *t, int sof, unsigned char *out)
{
	static const unsigned char soi_app0[] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 0x10, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
	const int grey = t->ncomp == 1;
	const mjw_plan *p = &t->plan;
	unsigned char *o = out;
#define PUT(src, n) (memcpy(o, (src), (n)), o += (n))
	PUT(soi_app0, sizeof(soi_app0));
	*o++ = 0xFF, *o++ = 0xDB, *o++ = 0, *o++ = (unsigned char)(grey ? 0x43 : 0x84), *o++ = 0;
	PUT(p->ytab, 64);
	if (!grey) {
		*o++ = 1;
		PUT(p->ctab, 64);
	}
	*o++ = 0xFF, *o++ = (unsigned char)sof, *o++ = 0, *o++ = (unsigned char)(grey ? 0x0B : 0x11), *o++ = 8;
	*o++ = (unsigned char)(p->height >> 8), *o++ = (unsigned char)(p->height & 0xff);
	*o++ = (unsigned char)(p->width >> 8), *o++ = (unsigned char)(p->width & 0xff);
	*o++ = (unsigned char)t->ncomp;
	*o++ = 1, *o++ = (unsigned char)(grey ? 0x11 : (t->lh << 4 | t->lv)), *o++ = 0;
	if (!grey) {
		*o++ = 2, *o++ = 0x11, *o++ = 1;
		*o++ = 3, *o++ = 0x11, *o++ = 1;
	}
#undef PUT
	return (size_t)(o - out);
}

/* SOI .. SOS with the four tables given as BITS (16 counts) and HUFFVAL, indexed luma DC, chroma DC, luma AC, chroma AC; a grey picture
 * carries only the two luma tables */
static size_t theader_tables(const mjw_tplan *t, const unsigned char *const bits[4], const unsigned char *const vals[4], unsigned char *out)
{
	static const unsigned char ids[4] = {0x00, 0x10, 0x01, 0x11};
	static const int order[4] = {0, 2, 1, 3};
	const int grey = t->ncomp == 1, ntab = grey ? 2 : 4;
	unsigned char *o = out + theader_frame(t, 0xC0, out), *dht_len;
	int k, i, n;
#define PUT(src, n) (memcpy(o, (src), (n)), o += (n))
	*o++ = 0xFF, *o++ = 0xC4;
	dht_len = o;
	o += 2;
	for (k = 0; k < ntab; ++k) {
		const int tb = order[k];
		for (i = 0, n = 0; i < 16; ++i)
			n += bits[tb][i];
		*o++ = ids[k];
		PUT(bits[tb], 16);
		PUT(vals[tb], (size_t)n);
	}
	n = (int)(o - dht_len);
	dht_len[0] = (unsigned char)(n >> 8);
	dht_len[1] = (unsigned char)(n & 0xff);
	if (grey) {
		static const unsigned char sos1[] = {0xFF, 0xDA, 0, 8, 1, 1, 0, 0, 0x3F, 0};
		PUT(sos1, sizeof(sos1));
	} else {
		static const unsigned char sos3[] = {0xFF, 0xDA, 0, 0xC, 3, 1, 0, 2, 0x11, 3, 0x11, 0, 0x3F, 0};
		PUT(sos3, sizeof(sos3));
	}
#undef PUT
	return (size_t)(o - out);
}

size_t mjw_theader(const mjw_tplan *t, unsigned char *out)
{
	const unsigned char *const bits[4] = {k_dc_lum_bits + 1, k_dc_chr_bits + 1, k_ac_lum_bits + 1, k_ac_chr_bits + 1};
	const unsigned char *const vals[4] = {k_dc_vals, k_dc_vals, k_ac_lum_vals, k_ac_chr_vals};
	return theader_tables(t, bits, vals, out);
}

size_t mjw_theader_optimized(const mjw_tplan *t, const uint8_t bits[4][16], const uint8_t vals[4][256], unsigned char *out)
{
	const unsigned char *const b[4] = {bits[0], bits[1], bits[2], bits[3]};
	const unsigned char *const v[4] = {vals[0], vals[1], vals[2], vals[3]};
	return theader_tables(t, b, v, out);
}

int mjw_tunits_codable(const mjw_tplan *t, const int16_t *du, const char **reason)
{
	const size_t nu = mjw_tplan_du_count(t);
	const int ny = tplan_ny(t), dpm = t->plan.du_per_mcu;
	int pred[3] = {0, 0, 0}, k;
	size_t u;
	for (u = 0; u < nu; ++u, du += 64) {
		const int p = (int)(u % (size_t)dpm), c = p < ny ? 0 : p - ny + 1, diff = du[0] - pred[c];
		pred[c] = du[0];
		if (diff < -2047 || diff > 2047) {
			if (reason)
				*reason = "a DC difference outside -2047..2047";
			return 0;
		}
		for (k = 1; k < 64; ++k)
			if (du[k] < -1023 || du[k] > 1023) {
				if (reason)
					*reason = "an AC coefficient outside -1023..1023";
				return 0;
			}
	}
	return 1;
}

int mjw_temit(const mjw_tplan *t, const int16_t *du, mjw_write_func *func, void *context)
{
	enc_table ydc, yac, cdc, cac;
	unsigned char hdr[MJW_HEADER_BYTES];
	if (!t || !func || !du || !mjw_tunits_codable(t, du, NULL))
		return 0;
	make_enc_table(&ydc, k_dc_lum_bits, k_dc_vals);
	make_enc_table(&cdc, k_dc_chr_bits, k_dc_vals);
	make_enc_table(&yac, k_ac_lum_bits, k_ac_lum_vals);
	make_enc_table(&cac, k_ac_chr_bits, k_ac_chr_vals);
	return emit_units_with((size_t)t->plan.mcu_x * (size_t)t->plan.mcu_y, tplan_ny(t), t->ncomp, 0, du, func, context, &ydc, &yac, &cdc, &cac, hdr,
								  mjw_theader(t, hdr));
}

int mjw_temit_optimized(const mjw_tplan *t, const int16_t *du, mjw_write_func *func, void *context)
{
	uint32_t freq[4][256];
	uint8_t bits[4][16], vals[4][256];
	unsigned char b17[17], hdr[MJW_HEADER_BYTES];
	enc_table tb[4];
	int k, n;
	if (!t || !func || !du || !mjw_tunits_codable(t, du, NULL))
		return 0;
	if (mjw_tplan_du_count(t) > (size_t)(UINT32_MAX / 64))
		return mjw_temit(t, du, func, context);
	histogram_units((size_t)t->plan.mcu_x * (size_t)t->plan.mcu_y, tplan_ny(t), t->ncomp, 0, du, freq);
	for (k = 0; k < 4; ++k) {
		memset(vals[k], 0, 256);
		if (!mjw_optimal_table(freq[k], bits[k], vals[k], &n))
			return mjw_temit(t, du, func, context); /* a code longer than 32 bits before limiting: the plain tables */
		b17[0] = 0;
		memcpy(b17 + 1, bits[k], 16);
		make_enc_table(&tb[k], b17, vals[k]);
	}
	return emit_units_with((size_t)t->plan.mcu_x * (size_t)t->plan.mcu_y, tplan_ny(t), t->ncomp, 0, du, func, context, &tb[0], &tb[2], &tb[1], &tb[3], hdr,
								  mjw_theader_optimized(t, bits, vals, hdr));
}

typedef struct {
	unsigned char *out;
	size_t cap, len;
	int overflow;
} mem_sink;
static void mem_sink_write(void *context, void *data, int size)
{
	mem_sink *m = (mem_sink *)context;
	if (m->len + (size_t)size > m->cap) {
		m->overflow = 1;
		return;
	}
	memcpy(m->out + m->len, data, (size_t)size);
	m->len += (size_t)size;
}
static size_t emit_to_memory(const mjw_plan *p, const int16_t *du, unsigned char *out, size_t cap, int optimize)
{
	mem_sink m;
	if (!p || !du || !out)
		return 0;
	m.out = out;
	m.cap = cap;
	m.len = 0;
	m.overflow = 0;
	if (!(optimize ? mjw_emit_optimized : mjw_emit)(p, du, mem_sink_write, &m) || m.overflow)
		return 0;
	return m.len;
}
size_t mjw_emit_to_memory(const mjw_plan *p, const int16_t *du, unsigned char *out, size_t cap) { return emit_to_memory(p, du, out, cap, 0); }
size_t mjw_emit_optimized_to_memory(const mjw_plan *p, const int16_t *du, unsigned char *out, size_t cap) { return emit_to_memory(p, du, out, cap, 1); }
size_t mjw_temit_to_memory(const mjw_tplan *t, const int16_t *du, unsigned flags, unsigned char *out, size_t cap)
{
	mem_sink m;
	if (!t || !du || !out)
		return 0;
	m.out = out;
	m.cap = cap;
	m.len = 0;
	m.overflow = 0;
	if (!((flags & MJW_OPTIMIZE_HUFFMAN) ? mjw_temit_optimized : mjw_temit)(t, du, mem_sink_write, &m) || m.overflow)
		return 0;
	return m.len;
}

/* ---- restart intervals (include/mij_host.h, RESTART INTERVALS): the same emission with a DRI segment in front of SOS, the scan's fill and
 * a marker at every interval end, and every quantity that follows the DC predictors taken against the restarted ones.  ri == 0 is the
 * calls above, byte for byte. */

int mjw_restart_interval(const mjw_tplan *t, int rows, int mcus, int *ri, const char **reason)
{
	const char *why = NULL;
	long long v = 0;
	if (!t || !ri || t->plan.mcu_x < 1 || t->plan.mcu_y < 1)
		why = "bad argument";
	else if (rows < 0 || mcus < 0)
		why = "a restart interval cannot be negative";
	else if (rows && mcus)
		why = "a restart interval is given in MCU rows or in MCUs, not both";
	else if ((v = rows ? (long long)rows * t->plan.mcu_x : mcus) > 65535)
		why = "a restart interval above 65535 MCUs does not fit the DRI segment";
	if (why) {
		if (reason)
			*reason = why;
		return 0;
	}
	*ri = (int)v;
	return 1;
}

/* the DRI segment pushed in between DHT and SOS of a finished header whose SOS segment takes sos_len bytes */
static size_t header_add_dri(unsigned char *hdr, size_t len, size_t sos_len, int ri)
{
	unsigned char *sos = hdr + len - sos_len;
	if (ri <= 0)
		return len;
	memmove(sos + 6, sos, sos_len);
	sos[0] = 0xFF, sos[1] = 0xDD, sos[2] = 0, sos[3] = 4;
	sos[4] = (unsigned char)(ri >> 8), sos[5] = (unsigned char)(ri & 0xff);
	return len + 6;
}
static int ri_ok(int ri) { return ri >= 0 && ri <= 65535; }
static size_t tplan_sos_len(const mjw_tplan *t) { return t->ncomp == 1 ? 10 : 14; }

size_t mjw_header_restart(const mjw_plan *p, int ri, unsigned char *out) { return ri_ok(ri) ? header_add_dri(out, mjw_header(p, out), 14, ri) : 0; }
size_t mjw_header_optimized_restart(const mjw_plan *p, const uint8_t bits[4][16], const uint8_t vals[4][256], int ri, unsigned char *out)
{
	return ri_ok(ri) ? header_add_dri(out, mjw_header_optimized(p, bits, vals, out), 14, ri) : 0;
}
size_t mjw_theader_restart(const mjw_tplan *t, int ri, unsigned char *out)
{
	return ri_ok(ri) ? header_add_dri(out, mjw_theader(t, out), tplan_sos_len(t), ri) : 0;
}
size_t mjw_theader_optimized_restart(const mjw_tplan *t, const uint8_t bits[4][16], const uint8_t vals[4][256], int ri, unsigned char *out)
{
	return ri_ok(ri) ? header_add_dri(out, mjw_theader_optimized(t, bits, vals, out), tplan_sos_len(t), ri) : 0;
}

int mjw_histogram_restart(const mjw_plan *p, const int16_t *du, int ri, uint32_t freq[4][256])
{
	if (!p || !du || !freq || !ri_ok(ri) || mjw_plan_du_count(p) > (size_t)(UINT32_MAX / 64))
		return 0;
	histogram_units((size_t)p->mcu_x * (size_t)p->mcu_y, p->subsample ? 4 : 1, 3, (size_t)ri, du, freq);
	return 1;
}
int mjw_thistogram_restart(const mjw_tplan *t, const int16_t *du, int ri, uint32_t freq[4][256])
{
	if (!t || !du || !freq || !ri_ok(ri) || mjw_tplan_du_count(t) > (size_t)(UINT32_MAX / 64))
		return 0;
	histogram_units((size_t)t->plan.mcu_x * (size_t)t->plan.mcu_y, tplan_ny(t), t->ncomp, (size_t)ri, du, freq);
	return 1;
}

/* mjw_tunits_codable's ranges over nm MCUs of ny luma units and, with three components, Cb and Cr; the predictors restart every ri MCUs */
static int units_codable(size_t nm, int ny, int ncomp, size_t ri, const int16_t *du, const char **reason)
{
	const int dpm = ny + (ncomp == 3 ? 2 : 0);
	int pred[3] = {0, 0, 0}, k, p;
	size_t m, left = ri;
	for (m = 0; m < nm; ++m) {
		for (p = 0; p < dpm; ++p, du += 64) {
			const int c = p < ny ? 0 : p - ny + 1, diff = du[0] - pred[c];
			pred[c] = du[0];
			if (diff < -2047 || diff > 2047) {
				if (reason)
					*reason = "a DC difference outside -2047..2047";
				return 0;
			}
			for (k = 1; k < 64; ++k)
				if (du[k] < -1023 || du[k] > 1023) {
					if (reason)
						*reason = "an AC coefficient outside -1023..1023";
					return 0;
				}
		}
		if (ri && --left == 0) {
			pred[0] = pred[1] = pred[2] = 0;
			left = ri;
		}
	}
	return 1;
}
int mjw_units_codable_restart(const mjw_plan *p, const int16_t *du, int ri, const char **reason)
{
	if (!p || !du || !ri_ok(ri)) {
		if (reason)
			*reason = "bad argument";
		return 0;
	}
	return units_codable((size_t)p->mcu_x * (size_t)p->mcu_y, p->subsample ? 4 : 1, 3, (size_t)ri, du, reason);
}
int mjw_tunits_codable_restart(const mjw_tplan *t, const int16_t *du, int ri, const char **reason)
{
	if (!t || !du || !ri_ok(ri)) {
		if (reason)
			*reason = "bad argument";
		return 0;
	}
	return units_codable((size_t)t->plan.mcu_x * (size_t)t->plan.mcu_y, tplan_ny(t), t->ncomp, (size_t)ri, du, reason);
}

/* the emission of a plan (t == NULL) or a transcode plan with an interval: plain tables, or the optimised ones of the restarted histogram (the
 * plain ones where a table cannot be built, as mjw_emit_optimized falls back) */
static int emit_restart(const mjw_plan *p, const mjw_tplan *t, const int16_t *du, unsigned flags, int ri, mjw_write_func *func, void *context)
{
	const size_t nm = (size_t)p->mcu_x * (size_t)p->mcu_y, nu = mjw_plan_du_count(p);
	const int ny = t ? tplan_ny(t) : (p->subsample ? 4 : 1), ncomp = t ? t->ncomp : 3;
	uint32_t freq[4][256];
	uint8_t bits[4][16], vals[4][256];
	unsigned char b17[17], hdr[MJW_HEADER_RESTART_BYTES];
	enc_table tb[4];
	size_t hlen;
	int k, n, opt = (flags & MJW_OPTIMIZE_HUFFMAN) && nu <= (size_t)(UINT32_MAX / 64);
	if (opt) {
		histogram_units(nm, ny, ncomp, (size_t)ri, du, freq);
		for (k = 0; k < 4 && opt; ++k) {
			memset(vals[k], 0, 256);
			if (!mjw_optimal_table(freq[k], bits[k], vals[k], &n)) {
				opt = 0;
				break;
			}
			b17[0] = 0;
			memcpy(b17 + 1, bits[k], 16);
			make_enc_table(&tb[k], b17, vals[k]);
		}
	}
	if (!opt) {
		make_enc_table(&tb[0], k_dc_lum_bits, k_dc_vals);
		make_enc_table(&tb[1], k_dc_chr_bits, k_dc_vals);
		make_enc_table(&tb[2], k_ac_lum_bits, k_ac_lum_vals);
		make_enc_table(&tb[3], k_ac_chr_bits, k_ac_chr_vals);
	}
	if (t)
		hlen = opt ? mjw_theader_optimized_restart(t, bits, vals, ri, hdr) : mjw_theader_restart(t, ri, hdr);
	else
		hlen = opt ? mjw_header_optimized_restart(p, bits, vals, ri, hdr) : mjw_header_restart(p, ri, hdr);
	return emit_units_with(nm, ny, ncomp, (size_t)ri, du, func, context, &tb[0], &tb[2], &tb[1], &tb[3], hdr, hlen);
}

int mjw_emit_restart(const mjw_plan *p, const int16_t *du, unsigned flags, int ri, mjw_write_func *func, void *context)
{
	if (!p || !du || !func || !ri_ok(ri) || (flags & ~MJW_OPTIMIZE_HUFFMAN))
		return 0;
	return emit_restart(p, NULL, du, flags, ri, func, context);
}
int mjw_temit_restart(const mjw_tplan *t, const int16_t *du, unsigned flags, int ri, mjw_write_func *func, void *context)
{
	if (!t || !du || !func || !ri_ok(ri) || (flags & ~MJW_OPTIMIZE_HUFFMAN) || !mjw_tunits_codable_restart(t, du, ri, NULL))
		return 0;
	return emit_restart(&t->plan, t, du, flags, ri, func, context);
}
size_t mjw_emit_restart_to_memory(const mjw_plan *p, const int16_t *du, unsigned flags, int ri, unsigned char *out, size_t cap)
{
	mem_sink m = {out, cap, 0, 0};
	if (!out || !mjw_emit_restart(p, du, flags, ri, mem_sink_write, &m) || m.overflow)
		return 0;
	return m.len;
}
size_t mjw_temit_restart_to_memory(const mjw_tplan *t, const int16_t *du, unsigned flags, int ri, unsigned char *out, size_t cap)
{
	mem_sink m = {out, cap, 0, 0};
	if (!out || !mjw_temit_restart(t, du, flags, ri, mem_sink_write, &m) || m.overflow)
		return 0;
	return m.len;
}

/* ---- progressive streams (include/mij_host.h, PROGRESSIVE STREAMS): the units coded scan after scan in libjpeg's jpeg_simple_progression
 * script, each scan under the optimal tables of its own symbol counts.  Every scan is walked twice: once counting, once writing. */

typedef struct {
	unsigned char ncomp, comp[3], ss, se, ah, al; /* comp: 0 luma, 1 Cb, 2 Cr */
} pg_scan;
static const pg_scan k_pg_colour[MJW_PROGRESSIVE_SCANS_COLOUR] = {
	{3, {0, 1, 2}, 0, 0, 0, 1}, {1, {0, 0, 0}, 1, 5, 0, 2},  {1, {2, 0, 0}, 1, 63, 0, 1}, {1, {1, 0, 0}, 1, 63, 0, 1}, {1, {0, 0, 0}, 6, 63, 0, 2},
	{1, {0, 0, 0}, 1, 63, 2, 1}, {3, {0, 1, 2}, 0, 0, 1, 0}, {1, {2, 0, 0}, 1, 63, 1, 0}, {1, {1, 0, 0}, 1, 63, 1, 0}, {1, {0, 0, 0}, 1, 63, 1, 0}};
static const pg_scan k_pg_grey[MJW_PROGRESSIVE_SCANS_GREY] = {{1, {0, 0, 0}, 0, 0, 0, 1}, {1, {0, 0, 0}, 1, 5, 0, 2},  {1, {0, 0, 0}, 6, 63, 0, 2},
																				  {1, {0, 0, 0}, 1, 63, 2, 1}, {1, {0, 0, 0}, 0, 0, 1, 0}, {1, {0, 0, 0}, 1, 63, 1, 0}};

typedef struct {
	jw_sink *s;          /* NULL while the scan's symbols are only counted */
	uint32_t *freq;      /* the table that counts / codes the next symbol */
	const enc_table *tb;
	unsigned eobrun, be; /* blocks of the pending end-of-band run; correction bits buffered behind it */
	unsigned char corr[MJW_PROGRESSIVE_MAX_CORR_BITS];
	mjw_progressive_stats *st;
} pg_state;

static inline void pg_symbol(pg_state *g, int sym)
{
	if (g->s)
		put_bits(g->s, g->tb->code[sym], g->tb->len[sym]);
	else
		++g->freq[sym];
}
static inline void pg_bits(pg_state *g, unsigned v, int n)
{
	if (g->s && n)
		put_bits(g->s, v & ((1u << n) - 1u), n);
}
static void pg_buffered(pg_state *g, const unsigned char *b, unsigned n)
{
	unsigned i;
	if (g->s)
		for (i = 0; i < n; ++i)
			put_bits(g->s, b[i], 1);
}
/* the pending run leaves: EOBn, the run's low n bits, then the correction bits that waited for it (jcphuff.c, emit_eobrun) */
static void pg_eobrun(pg_state *g)
{
	if (g->eobrun) {
		const int n = 31 - __builtin_clz(g->eobrun);
		if (g->st) {
			if (g->eobrun > g->st->longest_run)
				g->st->longest_run = g->eobrun;
			if (g->be > g->st->most_pending_bits)
				g->st->most_pending_bits = g->be;
		}
		pg_symbol(g, n << 4);
		pg_bits(g, g->eobrun, n);
		g->eobrun = 0;
		pg_buffered(g, g->corr, g->be);
		g->be = 0;
	}
}

/* AC first scan of one block (encode_mcu_AC_first): magnitudes shifted towards zero */
static void pg_ac_first(pg_state *g, const int16_t *blk, int ss, int se, int al)
{
	int k, r = 0;
	for (k = ss; k <= se; ++k) {
		const int v = blk[k];
		const unsigned a = (unsigned)(v < 0 ? -v : v) >> al;
		int n;
		if (!a) {
			++r;
			continue;
		}
		pg_eobrun(g);
		for (; r > 15; r -= 16)
			pg_symbol(g, 0xF0);
		n = 32 - __builtin_clz(a);
		pg_symbol(g, (r << 4) + n);
		pg_bits(g, v < 0 ? ~a : a, n);
		r = 0;
	}
	if (r > 0) {
		if (++g->eobrun == 0x7FFF) {
			if (g->st && !g->s)
				++g->st->forced_run_flushes;
			pg_eobrun(g);
		}
	}
}

/* AC refinement scan of one block (encode_mcu_AC_refine) */
static void pg_ac_refine(pg_state *g, const int16_t *blk, int ss, int se, int al)
{
	unsigned char absv[64], *br_buf = g->corr + g->be;
	unsigned br = 0;
	int k, r = 0, eob = 0;
	for (k = ss; k <= se; ++k) {
		const unsigned a = (unsigned)(blk[k] < 0 ? -blk[k] : blk[k]) >> al;
		absv[k] = (unsigned char)(a > 2 ? 2 | (a & 1) : a); /* all that is asked of it: zero, one, larger, and its low bit */
		if (a == 1)
			eob = k; /* the last newly non-zero coefficient */
	}
	for (k = ss; k <= se; ++k) {
		const unsigned a = absv[k];
		if (!a) {
			++r;
			continue;
		}
		while (r > 15 && k <= eob) { /* a ZRL is only worth writing in front of a newly non-zero coefficient */
			pg_eobrun(g);
			pg_symbol(g, 0xF0);
			r -= 16;
			pg_buffered(g, br_buf, br); /* the correction bits the sixteen zeros skipped over */
			br_buf = g->corr;
			br = 0;
		}
		if (a > 1) { /* already non-zero: one correction bit, behind the next symbol */
			br_buf[br++] = (unsigned char)(a & 1);
			continue;
		}
		pg_eobrun(g);
		pg_symbol(g, (r << 4) + 1);
		pg_bits(g, blk[k] < 0 ? 0 : 1, 1);
		pg_buffered(g, br_buf, br);
		br_buf = g->corr;
		br = 0;
		r = 0;
	}
	if (r > 0 || br > 0) { /* the block's trailing correction bits join the run's */
		++g->eobrun;
		g->be += br;
		if (g->eobrun == 0x7FFF || g->be > MJW_PROGRESSIVE_MAX_CORR_BITS - 64 + 1) {
			if (g->st && !g->s)
				++*(g->eobrun == 0x7FFF ? &g->st->forced_run_flushes : &g->st->forced_bit_flushes);
			pg_eobrun(g);
		}
	}
}

/* one scan over the units: DC scans MCU after MCU with every unit of the MCU, AC scans over the component's own ceil(w / 8) x ceil(h / 8)
 * blocks in raster order.  freq / tb: the scan's table 0 and, in the colour DC scan, the chroma table 1. */
static void pg_run_scan(pg_state *g, const mjw_tplan *t, const pg_scan *sc, const int16_t *du, uint32_t freq[2][256], const enc_table tb[2])
{
	const int ny = tplan_ny(t), dpm = t->plan.du_per_mcu;
	g->eobrun = g->be = 0;
	if (sc->ss == 0) {
		const size_t nm = (size_t)t->plan.mcu_x * (size_t)t->plan.mcu_y;
		int pred[3] = {0, 0, 0}, p;
		size_t m;
		for (m = 0; m < nm; ++m)
			for (p = 0; p < dpm; ++p, du += 64) {
				const int c = p < ny ? 0 : p - ny + 1;
				if (sc->ah) {
					pg_bits(g, (unsigned)(du[0] >> sc->al) & 1u, 1);
				} else {
					const int v = du[0] >> sc->al, diff = v - pred[c]; /* the shift is arithmetic: -1 >> 1 is -1 */
					unsigned bits = 0;
					int nbits = 0;
					pred[c] = v;
					if (diff)
						magnitude_bits(diff, &bits, &nbits);
					g->freq = freq[c ? 1 : 0];
					g->tb = &tb[c ? 1 : 0];
					pg_symbol(g, nbits);
					pg_bits(g, bits, nbits);
				}
			}
	} else {
		const int c = sc->comp[0], h = c ? 1 : t->lh, v = c ? 1 : t->lv, off = c ? ny + c - 1 : 0;
		const int bw = c || t->ncomp == 1 ? t->plan.mcu_x : (t->plan.width + 7) / 8, bh = c || t->ncomp == 1 ? t->plan.mcu_y : (t->plan.height + 7) / 8;
		const int hh = t->ncomp == 1 ? 1 : h, vv = t->ncomp == 1 ? 1 : v;
		int bx, by;
		g->freq = freq[0];
		g->tb = &tb[0];
		for (by = 0; by < bh; ++by)
			for (bx = 0; bx < bw; ++bx) {
				const int16_t *blk =
					du + 64 * (((size_t)(by / vv) * (size_t)t->plan.mcu_x + (size_t)(bx / hh)) * (size_t)dpm + (size_t)(off + (c ? 0 : (by % vv) * hh + bx % hh)));
				if (sc->ah)
					pg_ac_refine(g, blk, sc->ss, sc->se, sc->al);
				else
					pg_ac_first(g, blk, sc->ss, sc->se, sc->al);
			}
		pg_eobrun(g);
	}
}

static void pg_put_dht(jw_sink *s, int id, const uint8_t bits[16], const uint8_t *vals, int n)
{
	const unsigned char head[5] = {0xFF, 0xC4, (unsigned char)((19 + n) >> 8), (unsigned char)((19 + n) & 0xff), (unsigned char)id};
	sink_bytes(s, head, 5);
	sink_bytes(s, bits, 16);
	sink_bytes(s, vals, n);
}

static int plan_shape_ok(const mjw_tplan *t)
{
	return t && (t->ncomp == 1 || t->ncomp == 3) && t->plan.mcu_x > 0 && t->plan.mcu_y > 0 && t->plan.width > 0 && t->plan.height > 0 &&
			 (t->ncomp == 1 ? t->plan.du_per_mcu == 1 : (t->lh >= 1 && t->lh <= 2 && t->lv >= 1 && t->lv <= 2 && t->plan.du_per_mcu == t->lh * t->lv + 2)) &&
			 mjw_tplan_du_count(t) <= (size_t)(UINT32_MAX / 64);
}

static int emit_progressive(const mjw_tplan *t, const int16_t *du, mjw_write_func *func, void *context, mjw_progressive_stats *st)
{
	const pg_scan *script = t->ncomp == 1 ? k_pg_grey : k_pg_colour;
	const int nscan = t->ncomp == 1 ? MJW_PROGRESSIVE_SCANS_GREY : MJW_PROGRESSIVE_SCANS_COLOUR;
	unsigned char hdr[MJW_HEADER_BYTES];
	jw_sink *s = NULL;
	pg_state *g = (pg_state *)calloc(1, sizeof(*g));
	int i, k, ok = 0;
	if (!g)
		return 0;
	if (st)
		memset(st, 0, sizeof(*st));
	g->st = st;
	if (func) {
		s = (jw_sink *)calloc(1, sizeof(*s));
		if (!s)
			goto done;
		s->func = func;
		s->context = context;
		sink_bytes(s, hdr, (int)theader_frame(t, 0xC2, hdr));
	}
	for (i = 0; i < nscan; ++i) {
		const pg_scan *sc = &script[i];
		const int ntab = sc->ss == 0 ? (sc->ah ? 0 : (t->ncomp == 3 ? 2 : 1)) : 1;
		uint32_t freq[2][256];
		uint8_t bits[2][16], vals[2][256];
		unsigned char b17[17];
		enc_table tb[2];
		int n[2] = {0, 0};
		memset(freq, 0, sizeof(freq));
		g->s = NULL;
		pg_run_scan(g, t, sc, du, freq, tb);
		for (k = 0; k < ntab; ++k) {
			if (!mjw_optimal_table(freq[k], bits[k], vals[k], &n[k]))
				goto done; /* a code longer than 32 bits before limiting: no plain table knows the EOBn symbols */
			b17[0] = 0;
			memcpy(b17 + 1, bits[k], 16);
			make_enc_table(&tb[k], b17, vals[k]);
		}
		if (!s)
			continue;
		/* the scan's tables, each in a DHT segment of its own; AC tables: luma id 0, chroma id 1 */
		for (k = 0; k < ntab; ++k)
			pg_put_dht(s, sc->ss == 0 ? k : 0x10 | (sc->comp[0] ? 1 : 0), bits[k], vals[k], n[k]);
		sink_byte(s, 0xFF), sink_byte(s, 0xDA), sink_byte(s, 0), sink_byte(s, (unsigned char)(6 + 2 * sc->ncomp)), sink_byte(s, sc->ncomp);
		for (k = 0; k < sc->ncomp; ++k) {
			const int c = sc->comp[k], tbl = c ? 1 : 0;
			sink_byte(s, (unsigned char)(c + 1));
			sink_byte(s, (unsigned char)(sc->ss ? tbl : (sc->ah ? 0 : tbl << 4))); /* Td only in the first DC scan, Ta only in AC scans */
		}
		sink_byte(s, sc->ss), sink_byte(s, sc->se), sink_byte(s, (unsigned char)(sc->ah << 4 | sc->al));
		s->acc = 0;
		s->nacc = 0;
		g->s = s;
		pg_run_scan(g, t, sc, du, freq, tb);
		put_bits(s, 0x7F, 7); /* every scan ends as the baseline scan does */
		put_bits_finish(s);
	}
	if (s) {
		sink_byte(s, 0xFF);
		sink_byte(s, 0xD9);
		sink_flush(s);
	}
	ok = 1;
done:
	free(s);
	free(g);
	return ok;
}

size_t mjw_tframe_progressive(const mjw_tplan *t, unsigned char *out) { return plan_shape_ok(t) && out ? theader_frame(t, 0xC2, out) : 0; }

static void tplan_of_plan(mjw_tplan *t, const mjw_plan *p)
{
	t->plan = *p;
	t->ncomp = 3;
	t->lh = t->lv = p->subsample ? 2 : 1;
}

int mjw_temit_progressive(const mjw_tplan *t, const int16_t *du, mjw_write_func *func, void *context)
{
	if (!plan_shape_ok(t) || !du || !func || !mjw_tunits_codable(t, du, NULL))
		return 0;
	return emit_progressive(t, du, func, context, NULL);
}
int mjw_emit_progressive(const mjw_plan *p, const int16_t *du, mjw_write_func *func, void *context)
{
	mjw_tplan t;
	if (!p)
		return 0;
	tplan_of_plan(&t, p);
	return mjw_temit_progressive(&t, du, func, context);
}
int mjw_tprogressive_stats(const mjw_tplan *t, const int16_t *du, mjw_progressive_stats *st)
{
	if (!plan_shape_ok(t) || !du || !st || !mjw_tunits_codable(t, du, NULL))
		return 0;
	return emit_progressive(t, du, NULL, NULL, st);
}
size_t mjw_temit_progressive_to_memory(const mjw_tplan *t, const int16_t *du, unsigned char *out, size_t cap)
{
	mem_sink m = {out, cap, 0, 0};
	if (!out || !mjw_temit_progressive(t, du, mem_sink_write, &m) || m.overflow)
		return 0;
	return m.len;
}
size_t mjw_emit_progressive_to_memory(const mjw_plan *p, const int16_t *du, unsigned char *out, size_t cap)
{
	mem_sink m = {out, cap, 0, 0};
	if (!out || !mjw_emit_progressive(p, du, mem_sink_write, &m) || m.overflow)
		return 0;
	return m.len;
}

/* ---- sampled encoding (include/mij_host.h, SAMPLED ENCODING): the writer's transform over the five MCU shapes, under the tables of a
 * quality or given ones */

int mjw_splan_init(mjw_tplan *t, int width, int height, int comp, int quality, int ncomp, int lh, int lv, const unsigned char *luma,
                   const unsigned char *chroma)
{
	static const float aasf[8] = {1.0f * 2.828427125f,         1.387039845f * 2.828427125f, 1.306562965f * 2.828427125f, 1.175875602f * 2.828427125f,
											1.0f * 2.828427125f,         0.785694958f * 2.828427125f, 0.541196100f * 2.828427125f, 0.275899379f * 2.828427125f};
	mjw_plan *p;
	int row, col, k;
	if (!t || !mjw_plan_init(&t->plan, width, height, comp, quality) || !luma != !chroma)
		return 0;
	p = &t->plan;
	if (!ncomp) /* the writer's own choice for the quality */
		ncomp = 3, lh = lv = p->subsample ? 2 : 1;
	if (ncomp == 1 ? (lh != 1 || lv != 1) : (ncomp != 3 || lh < 1 || lh > 2 || lv < 1 || lv > 2))
		return 0;
	if (luma) {
		for (k = 0; k < 64; ++k)
			if (!luma[k] || !chroma[k])
				return 0;
		memcpy(p->ytab, luma, 64);
		memcpy(p->ctab, chroma, 64);
		for (row = 0, k = 0; row < 8; ++row)
			for (col = 0; col < 8; ++col, ++k) {
				p->fdtbl_y[k] = 1 / (p->ytab[k_zigzag_of[k]] * aasf[row] * aasf[col]);
				p->fdtbl_c[k] = 1 / (p->ctab[k_zigzag_of[k]] * aasf[row] * aasf[col]);
			}
	}
	t->ncomp = ncomp;
	t->lh = lh;
	t->lv = lv;
	p->subsample = ncomp == 3 && lh == 2 && lv == 2;
	p->mcu_x = (width + 8 * lh - 1) / (8 * lh);
	p->mcu_y = (height + 8 * lv - 1) / (8 * lv);
	p->du_per_mcu = ncomp == 1 ? 1 : lh * lv + 2;
	return 1;
}

void mjw_stransform_host(const mjw_tplan *t, const void *data, int flip, int16_t *du)
{
	const mjw_plan *p = &t->plan;
	const int width = p->width, height = p->height, comp = p->comp;
	const int og = comp > 2 ? 1 : 0, ob = comp > 2 ? 2 : 0;
	const unsigned char *px = (const unsigned char *)data;
	const int mw = 8 * t->lh, mh = 8 * t->lv, npx = mw * mh;
	int x, y, row, col, pos, i;
	float Y[128], U[128], V[128], R[128], G[128], B[128], su[64], sv[64];
	if (t->ncomp == 3 && t->lh == t->lv) { /* 4:2:0 and 4:4:4: the writer's own two shapes */
		mjw_transform_host(p, data, flip, du);
		return;
	}
	for (y = 0; y < height; y += mh)
		for (x = 0; x < width; x += mw) {
			for (row = y, pos = 0; row < y + mh; ++row) {
				int crow = row < height ? row : height - 1; /* replicate the last row / column */
				int base = (flip ? (height - 1 - crow) : crow) * width * comp;
				for (col = x; col < x + mw; ++col, ++pos) {
					int q = base + (col < width ? col : width - 1) * comp;
					R[pos] = px[q], G[pos] = px[q + og], B[pos] = px[q + ob];
				}
			}
			/* mjw_transform_host's expressions and association */
			for (pos = 0; pos < npx; pos += 4) {
				const __m128 r = _mm_loadu_ps(R + pos), g = _mm_loadu_ps(G + pos), b = _mm_loadu_ps(B + pos);
				_mm_storeu_ps(Y + pos, _mm_sub_ps(_mm_add_ps(_mm_add_ps(_mm_mul_ps(_mm_set1_ps(+0.29900f), r), _mm_mul_ps(_mm_set1_ps(0.58700f), g)),
																			  _mm_mul_ps(_mm_set1_ps(0.11400f), b)), _mm_set1_ps(128.0f)));
				if (t->ncomp == 1)
					continue;
				_mm_storeu_ps(U + pos, _mm_add_ps(_mm_sub_ps(_mm_mul_ps(_mm_set1_ps(-0.16874f), r), _mm_mul_ps(_mm_set1_ps(0.33126f), g)),
															 _mm_mul_ps(_mm_set1_ps(0.50000f), b)));
				_mm_storeu_ps(V + pos, _mm_sub_ps(_mm_sub_ps(_mm_mul_ps(_mm_set1_ps(+0.50000f), r), _mm_mul_ps(_mm_set1_ps(0.41869f), g)),
															 _mm_mul_ps(_mm_set1_ps(0.08131f), b)));
			}
			if (t->ncomp == 1) {
				transform_du(Y, 8, p->fdtbl_y, du);
				du += 64;
				continue;
			}
			if (t->lh == 2) { /* 4:2:2: 16 x 8 pixels, the mean of (left, right) */
				transform_du(Y + 0, 16, p->fdtbl_y, du);
				transform_du(Y + 8, 16, p->fdtbl_y, du + 64);
				for (i = 0; i < 64; ++i) {
					const int j = (i >> 3) * 16 + (i & 7) * 2;
					su[i] = (U[j] + U[j + 1]) * 0.5f;
					sv[i] = (V[j] + V[j + 1]) * 0.5f;
				}
			} else { /* 4:4:0: 8 x 16 pixels, the mean of (top, bottom) */
				transform_du(Y + 0, 8, p->fdtbl_y, du);
				transform_du(Y + 64, 8, p->fdtbl_y, du + 64);
				for (i = 0; i < 64; ++i) {
					const int j = (i >> 3) * 16 + (i & 7);
					su[i] = (U[j] + U[j + 8]) * 0.5f;
					sv[i] = (V[j] + V[j + 8]) * 0.5f;
				}
			}
			transform_du(su, 8, p->fdtbl_c, du + 128);
			transform_du(sv, 8, p->fdtbl_c, du + 192);
			du += 256;
		}
}

int mjh_write_jpg_sampled_to_memory(const void *pixels, int width, int height, int comp, int quality, int ncomp, int lh, int lv,
                                    const unsigned char *luma, const unsigned char *chroma, int flip, unsigned flags, int restart_mcus,
                                    int progressive, unsigned char **out, size_t *out_len)
{
	mjw_tplan t;
	int16_t *du;
	unsigned char *buf;
	size_t nu, cap, n;
	if (!pixels || !out || !out_len || (flags & ~MJW_OPTIMIZE_HUFFMAN) || !ri_ok(restart_mcus) || (progressive && restart_mcus) ||
		 !mjw_splan_init(&t, width, height, comp, quality, ncomp, lh, lv, luma, chroma))
		return 0;
	nu = mjw_tplan_du_count(&t);
	cap = progressive ? MJW_PROGRESSIVE_STREAM_CAP(nu) : MJW_STREAM_CAP(nu);
	du = (int16_t *)malloc(nu * 64 * sizeof(int16_t));
	buf = (unsigned char *)malloc(cap);
	if (!du || !buf) {
		free(du);
		free(buf);
		return 0;
	}
	mjw_stransform_host(&t, pixels, flip, du);
	n = progressive ? mjw_temit_progressive_to_memory(&t, du, buf, cap) : mjw_temit_restart_to_memory(&t, du, flags, restart_mcus, buf, cap);
	free(du);
	if (!n) {
		free(buf);
		return 0;
	}
	*out = buf;
	*out_len = n;
	return 1;
}

/* ---- plane encoding (include/mij_host.h, PLANE ENCODING): the writer behind its colour stage, fed with Y, Cb and Cr samples as they lie */

void mjw_video_range(mij_in_convert *cv)
{
	const double sy = 255.0 / 219.0, sc = 255.0 / 224.0;
	memset(cv, 0, sizeof(*cv));
	cv->dtype = MIJ_DT_U8;
	cv->scale[0] = (float)sy;
	cv->bias[0] = (float)(-16.0 * sy);
	cv->scale[1] = cv->scale[2] = (float)sc;
	cv->bias[1] = cv->bias[2] = (float)(128.0 - 128.0 * sc);
}

int mjw_pplan_init(mjw_tplan *t, int width, int height, int quality, int ncomp, int lh, int lv, const unsigned char *luma, const unsigned char *chroma)
{
	if (ncomp != 1 && ncomp != 3) /* the sampling is required: never the quality's choice */
		return 0;
	return mjw_splan_init(t, width, height, ncomp, quality, ncomp, lh, lv, luma, chroma);
}

/* what mjw_pplan_init made, and planes and a conversion that can be read */
static int planes_ok(const mjw_tplan *t, const mij_plane *pl, const mij_in_convert *cv)
{
	int c;
	if (!t || !pl || (t->ncomp != 1 && t->ncomp != 3) || t->plan.comp != t->ncomp)
		return 0;
	for (c = 0; c < 3; ++c) {
		if (c < t->ncomp ? (!pl[c].src || !pl[c].x_pitch) : pl[c].src != NULL)
			return 0;
		if (cv && c < t->ncomp && !(isfinite(cv->scale[c]) && isfinite(cv->bias[c])))
			return 0;
	}
	return !cv || cv->dtype == MIJ_DT_U8;
}

/* the contract's u for sample s of component c (mij.h, mij_in_convert): two roundings, no fused multiply-add (-ffp-contract=off) */
static unsigned char plane_convert(unsigned char s, const mij_in_convert *cv, int c)
{
	float t = (float)s * cv->scale[c];
	t = t + cv->bias[c];
	t = t > 0.0f ? t : 0.0f; /* fmaxf, fminf and rintf spelled without libm: a NaN fails the comparison and becomes 0 */
	t = t < 255.0f ? t : 255.0f;
	return (unsigned char)_mm_cvtss_si32(_mm_set_ss(t)); /* round half to even */
}

int mjw_ptransform_host(const mjw_tplan *t, const mij_plane *pl, const mij_in_convert *cv, int flip, int16_t *du)
{
	const mjw_plan *p;
	int c, mx, my, sx, sy, row, col, i;
	float blk[64];
	unsigned char lut[3][256];
	if (!planes_ok(t, pl, cv) || !du)
		return 0;
	p = &t->plan;
	for (c = 0; c < t->ncomp; ++c)
		for (i = 0; i < 256; ++i)
			lut[c][i] = cv ? plane_convert((unsigned char)i, cv, c) : (unsigned char)i;
	for (my = 0; my < p->mcu_y; ++my)
		for (mx = 0; mx < p->mcu_x; ++mx)
			for (c = 0; c < t->ncomp; ++c) {
				/* each plane on its own: its size, its blocks per MCU, its last column and row repeated */
				const int h = c ? 1 : t->lh, v = c ? 1 : t->lv;
				const int w = c ? (p->width + t->lh - 1) / t->lh : p->width, ht = c ? (p->height + t->lv - 1) / t->lv : p->height;
				const unsigned char *base = (const unsigned char *)pl[c].src;
				for (sy = 0; sy < v; ++sy)
					for (sx = 0; sx < h; ++sx) {
						for (row = 0; row < 8; ++row) {
							const int y = (my * v + sy) * 8 + row, cy = y < ht ? y : ht - 1;
							const unsigned char *line = base + (int64_t)(flip ? ht - 1 - cy : cy) * pl[c].row_pitch;
							for (col = 0; col < 8; ++col) {
								const int x = (mx * h + sx) * 8 + col;
								blk[8 * row + col] = (float)lut[c][line[(int64_t)(x < w ? x : w - 1) * pl[c].x_pitch]] - 128.0f;
							}
						}
						transform_du(blk, 8, c ? p->fdtbl_c : p->fdtbl_y, du);
						du += 64;
					}
			}
	return 1;
}

int mjh_write_jpg_planes_to_memory(const mij_plane *planes, int width, int height, int quality, int ncomp, int lh, int lv, const unsigned char *luma,
                                   const unsigned char *chroma, const mij_in_convert *cv, int flip, unsigned flags, int restart_mcus, int progressive,
                                   unsigned char **out, size_t *out_len)
{
	mjw_tplan t;
	int16_t *du;
	unsigned char *buf;
	size_t nu, cap, n;
	if (!planes || !out || !out_len || (flags & ~MJW_OPTIMIZE_HUFFMAN) || !ri_ok(restart_mcus) || (progressive && restart_mcus) ||
		 !mjw_pplan_init(&t, width, height, quality, ncomp, lh, lv, luma, chroma) || !planes_ok(&t, planes, cv))
		return 0;
	nu = mjw_tplan_du_count(&t);
	cap = progressive ? MJW_PROGRESSIVE_STREAM_CAP(nu) : MJW_STREAM_CAP(nu);
	du = (int16_t *)malloc(nu * 64 * sizeof(int16_t));
	buf = (unsigned char *)malloc(cap);
	if (!du || !buf) {
		free(du);
		free(buf);
		return 0;
	}
	mjw_ptransform_host(&t, planes, cv, flip, du);
	n = progressive ? mjw_temit_progressive_to_memory(&t, du, buf, cap) : mjw_temit_restart_to_memory(&t, du, flags, restart_mcus, buf, cap);
	free(du);
	if (!n) {
		free(buf);
		return 0;
	}
	*out = buf;
	*out_len = n;
	return 1;
}

/* ---- libjpeg encoding (include/mij_host.h, LIBJPEG ENCODING): libjpeg's default compression in integers, and its framing of the header */

int mjw_lj_plan_init(mjw_tplan *t, int width, int height, int comp, int quality, int ncomp, int lh, int lv, const unsigned char *luma,
                     const unsigned char *chroma)
{
	if (comp != 1 && comp != 3) /* libjpeg takes no grey + alpha and no RGBA rows */
		return 0;
	if (!ncomp) /* libjpeg's default sampling, whatever the quality */
		ncomp = 3, lh = lv = 2;
	if (ncomp == 3 && lh == 1 && lv == 2) /* "440": Pillow cannot write it, so nothing judges it */
		return 0;
	return mjw_splan_init(t, width, height, comp, quality, ncomp, lh, lv, luma, chroma);
}

uint32_t mjw_lj_quant_magic(int q) { return q < 1 || q > 255 ? 0u : (uint32_t)(((uint64_t)1 << 32) / (uint32_t)(8 * q)) + 1u; }

int mjw_lj_quantise(int x, int q)
{
	const uint32_t a = (uint32_t)(x < 0 ? -x : x) + 4u * (uint32_t)q;
	const int y = (int)(((uint64_t)a * mjw_lj_quant_magic(q)) >> 32); /* a div 8q, exact for a < 2^17 */
	return x < 0 ? -y : y;
}

void mjw_lj_quantise_all(int q, int32_t *out)
{
	int x;
	for (x = -32768; x <= 32768; ++x)
		out[x + 32768] = mjw_lj_quantise(x, q);
}

void mjw_lj_ycc(int r, int g, int b, unsigned char ycc[3])
{
	ycc[0] = (unsigned char)((19595 * r + 38470 * g + 7471 * b + 32768) >> 16);
	ycc[1] = (unsigned char)((-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16);
	ycc[2] = (unsigned char)((32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16);
}

#define LJ_D(x, n) (((x) + (1 << ((n) - 1))) >> (n))
/* jfdctint.c's pass over d[0], d[s], .. d[7s] in place: the first pass (rows) scales up by 4, the second (columns) descales */
static void lj_fdct8(int32_t *d, int s, int first)
{
	const int n = first ? 11 : 15;
	int32_t t0 = d[0] + d[7 * s], t7 = d[0] - d[7 * s], t1 = d[s] + d[6 * s], t6 = d[s] - d[6 * s];
	int32_t t2 = d[2 * s] + d[5 * s], t5 = d[2 * s] - d[5 * s], t3 = d[3 * s] + d[4 * s], t4 = d[3 * s] - d[4 * s];
	const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
	int32_t z1, z2, z3, z4, z5;
	d[0] = first ? (t10 + t11) * 4 : LJ_D(t10 + t11, 2);
	d[4 * s] = first ? (t10 - t11) * 4 : LJ_D(t10 - t11, 2);
	z1 = (t12 + t13) * 4433;
	d[2 * s] = LJ_D(z1 + t13 * 6270, n);
	d[6 * s] = LJ_D(z1 - t12 * 15137, n);
	z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
	z5 = (z3 + z4) * 9633;
	t4 *= 2446, t5 *= 16819, t6 *= 25172, t7 *= 12299;
	z1 *= -7373, z2 *= -20995;
	z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
	d[7 * s] = LJ_D(t4 + z1 + z3, n);
	d[5 * s] = LJ_D(t5 + z2 + z4, n);
	d[3 * s] = LJ_D(t6 + z2 + z3, n);
	d[s] = LJ_D(t7 + z1 + z4, n);
}

/* one block of samples (pitch bytes between rows) -> its unit under table tab (zigzag order) */
static void lj_block(const unsigned char *src, size_t pitch, const unsigned char *tab, int16_t *du)
{
	int32_t d[64];
	int i;
	for (i = 0; i < 64; ++i)
		d[i] = (int32_t)src[(size_t)(i >> 3) * pitch + (size_t)(i & 7)] - 128;
	for (i = 0; i < 8; ++i)
		lj_fdct8(d + 8 * i, 1, 1);
	for (i = 0; i < 8; ++i)
		lj_fdct8(d + i, 8, 0);
	for (i = 0; i < 64; ++i) {
		const int z = k_zigzag_of[i];
		du[z] = (int16_t)mjw_lj_quantise(d[i], tab[z]);
	}
}

size_t mjw_lj_staged_bytes(const mjw_tplan *t)
{
	return t ? (size_t)t->plan.mcu_x * (size_t)t->plan.mcu_y * (size_t)t->plan.du_per_mcu * 64 : 0;
}

/* pass 2: the staged planes (Y of 8 lh mcu_x x 8 lv mcu_y samples, then Cb, then Cr of 8 mcu_x x 8 mcu_y) -> the units, dummy blocks by rule */
int mjw_lj_units_from_staged(const mjw_tplan *t, const unsigned char *staged, int16_t *du)
{
	const mjw_plan *p;
	int lh, lv, rw, rh, mx, my, sx, sy, c;
	size_t ypitch, cpitch, ybytes, cbytes;
	if (!t || !staged || !du || (t->ncomp != 1 && t->ncomp != 3))
		return 0;
	p = &t->plan;
	lh = t->ncomp == 1 ? 1 : t->lh, lv = t->ncomp == 1 ? 1 : t->lv;
	rw = (p->width + 7) / 8, rh = (p->height + 7) / 8;
	ypitch = (size_t)p->mcu_x * 8 * (size_t)lh, cpitch = (size_t)p->mcu_x * 8;
	ybytes = ypitch * (size_t)p->mcu_y * 8 * (size_t)lv, cbytes = cpitch * (size_t)p->mcu_y * 8;
	for (my = 0; my < p->mcu_y; ++my)
		for (mx = 0; mx < p->mcu_x; ++mx) {
			int16_t *const mcu = du;
			for (sy = 0; sy < lv; ++sy)
				for (sx = 0; sx < lh; ++sx, du += 64) {
					const int bx = mx * lh + sx, by = my * lv + sy;
					if (bx < rw && by < rh) {
						lj_block(staged + ((size_t)by * 8) * ypitch + (size_t)bx * 8, ypitch, p->ytab, du);
						continue;
					}
					/* a dummy block: no AC, the DC of the block before it -- its left neighbour in a real block row, the last block
					 * of the MCU's previous block row anywhere in a row below the picture */
					memset(du, 0, 64 * sizeof(int16_t));
					du[0] = by < rh ? du[-64] : mcu[((sy - 1) * lh + lh - 1) * 64];
				}
			for (c = 1; c < t->ncomp; ++c, du += 64)
				lj_block(staged + ybytes + (size_t)(c - 1) * cbytes + ((size_t)my * 8) * cpitch + (size_t)mx * 8, cpitch, p->ctab, du);
		}
	return 1;
}

/* pass 1: pixels -> the staged planes: the colour conversion, the column and row rules, the chroma filter */
int mjw_lj_stage_host(const mjw_tplan *t, const void *data, int flip, unsigned char *staged)
{
	const mjw_plan *p;
	const unsigned char *px = (const unsigned char *)data;
	int lh, lv, W, H, CW, CH, x, y, c, comp, rows, width, height;
	unsigned char *Y, *full;
	if (!t || !data || !staged || (t->ncomp != 1 && t->ncomp != 3) || (t->plan.comp != 1 && t->plan.comp != 3))
		return 0;
	p = &t->plan;
	comp = p->comp, width = p->width, height = p->height;
	lh = t->ncomp == 1 ? 1 : t->lh, lv = t->ncomp == 1 ? 1 : t->lv;
	W = p->mcu_x * 8 * lh, H = p->mcu_y * 8 * lv, CW = p->mcu_x * 8, CH = p->mcu_y * 8;
	rows = (height + lv - 1) / lv * lv; /* the pixel rows a chroma filter reads */
	Y = staged;
	full = (unsigned char *)malloc((size_t)W * (size_t)rows * 2); /* Cb and Cr at full size, columns extended */
	if (!full)
		return 0;
	for (y = 0; y < H; ++y) {
		const int cy = y < height ? y : height - 1;
		const unsigned char *line = px + (size_t)(flip ? height - 1 - cy : cy) * (size_t)width * (size_t)comp;
		for (x = 0; x < W; ++x) {
			const unsigned char *q = line + (size_t)(x < width ? x : width - 1) * (size_t)comp;
			unsigned char ycc[3];
			mjw_lj_ycc(q[0], q[comp > 2 ? 1 : 0], q[comp > 2 ? 2 : 0], ycc);
			Y[(size_t)y * W + x] = ycc[0];
			if (y < rows) {
				full[(size_t)y * W + x] = ycc[1];
				full[(size_t)(rows + y) * W + x] = ycc[2];
			}
		}
	}
	for (c = 0; c < t->ncomp - 1; ++c) {
		const unsigned char *src = full + (size_t)c * (size_t)rows * W;
		unsigned char *dst = staged + (size_t)W * H + (size_t)c * (size_t)CW * CH;
		const int srows = rows / lv;
		for (y = 0; y < CH; ++y) {
			const unsigned char *a = src + (size_t)(y < srows ? y : srows - 1) * lv * W, *b = a + W; /* the last SAMPLE row repeated */
			for (x = 0; x < CW; ++x)
				dst[(size_t)y * CW + x] = lh == 1   ? a[x]
				                          : lv == 1 ? (unsigned char)((a[2 * x] + a[2 * x + 1] + (x & 1)) >> 1)
				                                    : (unsigned char)((a[2 * x] + a[2 * x + 1] + b[2 * x] + b[2 * x + 1] + 1 + (x & 1)) >> 2);
		}
	}
	free(full);
	return 1;
}

int mjw_lj_transform_host(const mjw_tplan *t, const void *pixels, int flip, int16_t *du)
{
	unsigned char *staged = t ? (unsigned char *)malloc(mjw_lj_staged_bytes(t)) : NULL;
	const int ok = staged && mjw_lj_stage_host(t, pixels, flip, staged) && mjw_lj_units_from_staged(t, staged, du);
	free(staged);
	return ok;
}

/* mjw_ptransform_host's staging (each plane extended on its own by its last column and row), then pass 2 */
int mjw_lj_ptransform_host(const mjw_tplan *t, const mij_plane *pl, const mij_in_convert *cv, int flip, int16_t *du)
{
	unsigned char *staged, *dst;
	unsigned char lut[256];
	int c, x, y, i, ok;
	if (!planes_ok(t, pl, cv) || !du || (t->ncomp == 3 && t->lh == 1 && t->lv == 2))
		return 0;
	staged = dst = (unsigned char *)malloc(mjw_lj_staged_bytes(t));
	if (!staged)
		return 0;
	for (c = 0; c < t->ncomp; ++c) {
		const int h = c ? 1 : t->lh, v = c ? 1 : t->lv;
		const int w = c ? (t->plan.width + t->lh - 1) / t->lh : t->plan.width, ht = c ? (t->plan.height + t->lv - 1) / t->lv : t->plan.height;
		const int pw = t->plan.mcu_x * 8 * h, ph = t->plan.mcu_y * 8 * v;
		for (i = 0; i < 256; ++i)
			lut[i] = cv ? plane_convert((unsigned char)i, cv, c) : (unsigned char)i;
		for (y = 0; y < ph; ++y) {
			const int cy = y < ht ? y : ht - 1;
			const unsigned char *line = (const unsigned char *)pl[c].src + (int64_t)(flip ? ht - 1 - cy : cy) * pl[c].row_pitch;
			for (x = 0; x < pw; ++x)
				dst[(size_t)y * pw + x] = lut[line[(int64_t)(x < w ? x : w - 1) * pl[c].x_pitch]];
		}
		dst += (size_t)pw * ph;
	}
	ok = mjw_lj_units_from_staged(t, staged, du);
	free(staged);
	return ok;
}

/* `len` bytes that start with SOI and run at least to the first SOS marker, in libjpeg's framing: every DQT and DHT segment before that
 * SOS split into one segment per table; everything else, and everything from SOS on, as it is.  Returns the new length (at most
 * len + 4 per table), 0 for a malformed segment. */
size_t mjw_lj_reframe(const unsigned char *in, size_t len, unsigned char *out)
{
	size_t i = 2, o = 2;
	if (!in || !out || len < 4 || in[0] != 0xFF || in[1] != 0xD8)
		return 0;
	out[0] = 0xFF, out[1] = 0xD8;
	while (i + 4 <= len && in[i] == 0xFF && in[i + 1] != 0xDA) {
		const int marker = in[i + 1];
		const size_t seg = (size_t)in[i + 2] << 8 | in[i + 3], end = i + 2 + seg;
		if (seg < 2 || end > len)
			return 0;
		if (marker != 0xDB && marker != 0xC4) {
			memcpy(out + o, in + i, 2 + seg);
			o += 2 + seg;
			i = end;
			continue;
		}
		for (i += 4; i < end;) {
			size_t n = 65; /* DQT: Pq / Tq and 64 bytes (eight-bit tables only) */
			int k;
			if (marker == 0xC4) {
				if (i + 17 > end)
					return 0;
				for (k = 0, n = 17; k < 16; ++k)
					n += in[i + 1 + k];
			} else if (in[i] >> 4) {
				return 0;
			}
			if (i + n > end)
				return 0;
			out[o++] = 0xFF, out[o++] = (unsigned char)marker, out[o++] = (unsigned char)((n + 2) >> 8), out[o++] = (unsigned char)((n + 2) & 0xff);
			memcpy(out + o, in + i, n);
			o += n;
			i += n;
		}
	}
	if (i + 2 > len || in[i] != 0xFF || in[i + 1] != 0xDA)
		return 0;
	memcpy(out + o, in + i, len - i);
	return o + (len - i);
}

size_t mjw_lj_theader_restart(const mjw_tplan *t, int ri, unsigned char *out)
{
	unsigned char hdr[MJW_HEADER_RESTART_BYTES];
	const size_t n = t && out ? mjw_theader_restart(t, ri, hdr) : 0;
	return n ? mjw_lj_reframe(hdr, n, out) : 0;
}

size_t mjw_lj_theader_optimized_restart(const mjw_tplan *t, const uint8_t bits[4][16], const uint8_t vals[4][256], int ri, unsigned char *out)
{
	unsigned char hdr[MJW_HEADER_RESTART_BYTES];
	const size_t n = t && out ? mjw_theader_optimized_restart(t, bits, vals, ri, hdr) : 0;
	return n ? mjw_lj_reframe(hdr, n, out) : 0;
}

/* SOI .. SOF2: the progressive frame header with a DQT segment per table (there is no SOS to stop at: the same walk to the end) */
size_t mjw_lj_tframe_progressive(const mjw_tplan *t, unsigned char *out)
{
	unsigned char hdr[MJW_HEADER_RESTART_BYTES + 2];
	size_t n = t && out ? mjw_tframe_progressive(t, hdr) : 0;
	if (!n)
		return 0;
	hdr[n] = 0xFF, hdr[n + 1] = 0xDA;
	n = mjw_lj_reframe(hdr, n + 2, out);
	return n ? n - 2 : 0;
}

int mjh_write_jpg_libjpeg_to_memory(const void *pixels, int width, int height, int comp, int quality, int ncomp, int lh, int lv,
                                    const unsigned char *luma, const unsigned char *chroma, int flip, unsigned flags, int restart_mcus,
                                    int progressive, unsigned char **out, size_t *out_len)
{
	mjw_tplan t;
	int16_t *du;
	unsigned char *buf, *res;
	size_t nu, cap, n;
	if (!pixels || !out || !out_len || (flags & ~MJW_OPTIMIZE_HUFFMAN) || !ri_ok(restart_mcus) || (progressive && restart_mcus) ||
		 !mjw_lj_plan_init(&t, width, height, comp, quality, ncomp, lh, lv, luma, chroma))
		return 0;
	nu = mjw_tplan_du_count(&t);
	cap = progressive ? MJW_PROGRESSIVE_STREAM_CAP(nu) : MJW_STREAM_CAP(nu);
	du = (int16_t *)malloc(nu * 64 * sizeof(int16_t));
	buf = (unsigned char *)malloc(cap);
	res = (unsigned char *)malloc(cap + MJW_LJ_HEADER_EXTRA);
	n = 0;
	if (du && buf && res && mjw_lj_transform_host(&t, pixels, flip, du)) {
		n = progressive ? mjw_temit_progressive_to_memory(&t, du, buf, cap) : mjw_temit_restart_to_memory(&t, du, flags, restart_mcus, buf, cap);
		n = n ? mjw_lj_reframe(buf, n, res) : 0;
	}
	free(du);
	free(buf);
	if (!n) {
		free(res);
		return 0;
	}
	*out = res;
	*out_len = n;
	return 1;
}

int stbi_write_jpg_to_func(stbi_write_func *func, void *context, int x, int y, int comp, const void *data, int quality)
{
	mjw_plan plan;
	int16_t *du;
	int ok;
	if (!func || !data)
		return 0;
	if (!mjw_plan_init(&plan, x, y, comp, quality))
		return 0;
	du = (int16_t *)malloc(mjw_plan_du_count(&plan) * 64 * sizeof(int16_t));
	if (!du)
		return 0;
	mjw_transform_host(&plan, data, g_flip_on_write, du);
	ok = mjw_emit(&plan, du, func, context);
	free(du);
	return ok;
}

int mjw_flip_on_write(void) { return g_flip_on_write; }

static void file_sink(void *context, void *data, int size) { fwrite(data, 1, (size_t)size, (FILE *)context); }

int stbi_write_jpg(char const *filename, int x, int y, int comp, const void *data, int quality)
{
	FILE *f = fopen(filename, "wb");
	int ok;
	if (!f)
		return 0;
	ok = stbi_write_jpg_to_func(file_sink, f, x, y, comp, data, quality);
	fclose(f);
	return ok;
}
