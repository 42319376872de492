/* The optimised-table pieces of the host writer (mjw_histogram, mjw_optimal_table, mjw_header_optimized, mjw_emit_optimized,
 * mjw_emit_optimized_to_memory: image-codecs_amd/csrc/jpeg_write_host.c) under AddressSanitizer + UBSan (CPU build only;
 * tests/test_encode_optimize_host.py builds and runs this).  Every buffer is a heap block of exactly the size the interface names, so a
 * read or write past it is reported:
 *   - pictures of several sizes, channel counts and qualities: units in an exact-size block, the optimised stream emitted twice
 *     (byte-equal), shorter than or as long as the header bound allows, emitted into memory with the exact capacity and refused
 *     with one byte less;
 *   - mjw_optimal_table on exact-size blocks: random counts, one symbol, no symbol, 256 equal counts, counts of 2^32 - 1, and
 *     Fibonacci-like chains of depth 16, 17, 32 (shortened to 16 bits) and 33 (returns 0).
 * Exit status 0 only when every check held. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "image_api.h"
#include "mij_host.h"

typedef struct { unsigned char *p; size_t n, cap; } sink;
static void sink_write(void *ctx, void *data, int size)
{
	sink *s = (sink *)ctx;
	if (s->n + (size_t)size > s->cap) { s->cap = (s->n + (size_t)size) * 2; s->p = realloc(s->p, s->cap); }
	memcpy(s->p + s->n, data, (size_t)size);
	s->n += (size_t)size;
}
static uint32_t lcg(uint32_t *s) { *s = *s * 1664525u + 1013904223u; return *s >> 8; }

static int bad = 0;
#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); ++bad; } } while (0)

/* mjw_optimal_table on exact-size blocks; returns its result, *longest = the longest code, *n = the symbols */
static int table(const uint32_t *counts, int *longest, int *n)
{
	uint32_t *freq = malloc(256 * sizeof *freq);
	uint8_t *bits = malloc(16), *vals = malloc(256);
	int ok, i, sum = 0;
	unsigned kraft = 0;
	memcpy(freq, counts, 256 * sizeof *freq);
	ok = mjw_optimal_table(freq, bits, vals, n);
	*longest = 0;
	if (ok) {
		for (i = 0; i < 16; ++i) {
			sum += bits[i];
			kraft += (unsigned)bits[i] << (15 - i);
			if (bits[i])
				*longest = i + 1;
		}
		CHECK(sum == *n, "BITS sum %d != %d symbols", sum, *n);
		CHECK(kraft < 65536u, "codes do not leave the all-ones code free"); /* the pseudo-symbol's place */
		for (i = 0; i < *n; ++i)
			CHECK(counts[vals[i]] != 0, "HUFFVAL lists symbol %d, which has no count", vals[i]);
	}
	free(freq); free(bits); free(vals);
	return ok;
}

static void chain(uint32_t *f, int depth)
{
	uint64_t total = 4;
	int k;
	memset(f, 0, 256 * sizeof *f);
	f[3] = 1;
	f[10] = 2;
	for (k = 2; k < depth; ++k) {
		const uint32_t prev = f[3 + 7 * (k - 1)], c = (uint32_t)(total - prev + 1);
		f[3 + 7 * k] = c;
		total += c;
	}
}

typedef struct { int w, h, comp, q, kind; } pic;

int main(void)
{
	static const pic cases[] = {{1, 1, 3, 90, 0}, {17, 33, 3, 75, 0}, {33, 17, 1, 50, 1}, {64, 64, 3, 90, 3}, {97, 51, 4, 95, 0},
										 {250, 3, 2, 100, 2}, {129, 65, 3, 91, 1}, {320, 240, 3, 90, 0}, {16, 16, 3, 0, 2}};
	const int n = (int)(sizeof cases / sizeof cases[0]);
	uint32_t f[256], seed = 7;
	int k, i, longest, nv;
	for (k = 0; k < n; ++k) {
		const pic *c = &cases[k];
		const size_t npx = (size_t)c->w * c->h * c->comp;
		unsigned char *px = malloc(npx), *mem;
		uint32_t (*freq)[256] = malloc(4 * 256 * sizeof(uint32_t));
		mjw_plan plan;
		int16_t *du;
		size_t elems, t, len;
		sink a = {0}, b = {0}, plain = {0};
		for (t = 0; t < npx; ++t) {
			const uint32_t r = lcg(&seed);
			px[t] = c->kind == 0 ? (unsigned char)r : c->kind == 1 ? (unsigned char)((t * 7 / (size_t)c->comp) & 255) : c->kind == 2 ? (unsigned char)((r & 1) ? 255 : 0) : 128;
		}
		CHECK(mjw_plan_init(&plan, c->w, c->h, c->comp, c->q), "case %d: plan refused", k);
		elems = mjw_plan_du_count(&plan) * 64;
		du = malloc(elems * sizeof(int16_t));
		mjw_transform_host(&plan, px, 0, du);
		CHECK(mjw_histogram(&plan, du, freq), "case %d: histogram refused", k);
		for (t = 0, len = 0; t < 256; ++t)
			len += freq[0][t] + freq[1][t];
		CHECK(len == elems / 64, "case %d: %zu DC symbols for %zu units", k, len, elems / 64);
		CHECK(mjw_emit_optimized(&plan, du, sink_write, &a) && mjw_emit_optimized(&plan, du, sink_write, &b), "case %d: emission failed", k);
		CHECK(a.n == b.n && !memcmp(a.p, b.p, a.n), "case %d: second emission differs", k);
		CHECK(mjw_emit(&plan, du, sink_write, &plain), "case %d: plain emission failed", k);
		CHECK(a.n >= 4 && a.p[0] == 0xFF && a.p[1] == 0xD8 && a.p[a.n - 2] == 0xFF && a.p[a.n - 1] == 0xD9, "case %d: no SOI / EOI", k);
		mem = malloc(a.n);
		CHECK(mjw_emit_optimized_to_memory(&plan, du, mem, a.n) == a.n && !memcmp(mem, a.p, a.n), "case %d: emission to memory differs", k);
		CHECK(mjw_emit_optimized_to_memory(&plan, du, mem, a.n - 1) == 0, "case %d: a capacity one byte short was accepted", k);
		printf("case %d: %zu -> %zu bytes\n", k, plain.n, a.n);
		free(mem); free(a.p); free(b.p); free(plain.p); free(du); free(freq); free(px);
	}
	for (k = 0; k < 200; ++k) { /* random counts, from dense to sparse */
		for (i = 0; i < 256; ++i)
			f[i] = (lcg(&seed) % 7u) < (uint32_t)(k % 7) ? 0u : (lcg(&seed) << 8 | lcg(&seed)) >> (k % 31);
		CHECK(table(f, &longest, &nv) && longest <= 16, "random histogram %d refused", k);
	}
	memset(f, 0, sizeof f);
	CHECK(table(f, &longest, &nv) && nv == 0, "no symbol: %d symbols", nv);
	f[200] = 1;
	CHECK(table(f, &longest, &nv) && nv == 1 && longest == 1, "one symbol: %d symbols, %d bits", nv, longest);
	for (i = 0; i < 256; ++i)
		f[i] = 1;
	CHECK(table(f, &longest, &nv) && nv == 256 && longest == 9, "256 equal counts: %d symbols, %d bits", nv, longest);
	for (i = 0; i < 256; ++i)
		f[i] = 0xFFFFFFFFu;
	CHECK(table(f, &longest, &nv) && nv == 256, "largest counts refused");
	for (k = 0; k < 4; ++k) {
		static const int depth[4] = {16, 17, 32, 33};
		chain(f, depth[k]);
		i = table(f, &longest, &nv);
		if (depth[k] <= 32)
			CHECK(i && nv == depth[k] && longest == 16, "chain of depth %d: ok %d, %d symbols, %d bits", depth[k], i, nv, longest);
		else
			CHECK(!i, "chain of depth %d was not refused", depth[k]);
	}
	printf("hufopt harness: %d failures\n", bad);
	return bad ? 1 : 0;
}
