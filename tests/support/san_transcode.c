/* The host half of the lossless transcode (image-codecs_amd/csrc/transcode_host.c and the mjw_temit* calls of jpeg_write_host.c) under
 * AddressSanitizer + UBSan, as a stand-alone CPU program (tests/test_transcode_host.py builds and runs it).  For the five MCU shapes and
 * sizes that are no MCU multiple it
 *   - fills coefficient planes in both formats, in heap blocks of exactly the region's size, with values up to the codable limits
 *     (escaped blocks included), reads them as units into a block of exactly the units' size and requires both formats to agree,
 *   - emits plain and optimised streams, to a callback and to memory, and requires them to be equal,
 *   - runs mjh_transcode_memory on the plain stream (it must return the stream itself: a fixed point) and on EVERY prefix of it,
 *   - splices markers from sources with segments, and from every prefix of such a source.
 * Exit status 0 only when every comparison held. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
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

static void make_desc(mij_image_desc *d, int w, int h, int ncomp, int lh, int lv)
{
	int c, i;
	memset(d, 0, sizeof(*d));
	d->width = w, d->height = h, d->ncomp = ncomp, d->n_out = ncomp, d->color = ncomp == 3 ? MIJ_COLOR_YCBCR : MIJ_COLOR_GREY;
	d->h_max = lh, d->v_max = lv;
	d->mcu_x = (w + 8 * lh - 1) / (8 * lh), d->mcu_y = (h + 8 * lv - 1) / (8 * lv);
	for (c = 0; c < ncomp; ++c) {
		mij_comp_desc *cp = &d->comp[c];
		cp->h = c ? 1 : lh, cp->v = c ? 1 : lv, cp->tq = c ? 1 : 0;
		cp->bw = d->mcu_x * cp->h, cp->bh = d->mcu_y * cp->v;
		cp->x = (w * cp->h + lh - 1) / lh, cp->y = (h * cp->v + lv - 1) / lv;
	}
	for (i = 0; i < 64; ++i)
		d->dequant[0][i] = (uint16_t)(1 + i % 7), d->dequant[1][i] = (uint16_t)(255 - i);
}

/* one coefficient into both regions */
static void put(const mij_image_desc *d, uint8_t *r16, uint8_t *rc, int c, uint32_t L, int P, int v)
{
	size_t off = 0, lo, dc, hi;
	int k;
	for (k = 0; k < c; ++k)
		off += mij_plane_elems((uint32_t)(d->comp[k].bw * d->comp[k].bh)) * 2;
	((int16_t *)(void *)(r16 + off))[mij_coef_index(L, (uint32_t)P)] = (int16_t)v;
	mij_compact_offsets(d, c, &lo, &dc, &hi);
	if (P == 0) {
		int16_t s = (int16_t)v;
		memcpy(rc + dc + 2 * (size_t)L, &s, 2);
		return;
	}
	{
		uint8_t *blo = rc + lo + (((size_t)L >> 6) << 12) + (((size_t)L & 63) << 3);
		blo[((size_t)(P >> 3) << 9) + (P & 7)] = (uint8_t)(v & 255);
		if (v < -128 || v > 127) {
			if (!(blo[0] & 1)) { /* first escape of the block: its 64 escape bytes become defined */
				memset(rc + hi + ((size_t)L << 6), 0, 64); /* sext8(low byte) + 256 * 0 is what the plain bytes already say */
				blo[0] |= 1;
			}
		}
		if (blo[0] & 1)
			rc[hi + ((size_t)L << 6) + (size_t)P] = (uint8_t)(((v - (int8_t)(v & 255)) >> 8) & 255);
	}
}

static int check_prefixes(const unsigned char *s, size_t n)
{
	size_t k;
	int bad = 0;
	for (k = 0; k < n; k += (k < 700 || n - k < 40) ? 1 : 37) {
		unsigned char *copy = malloc(k ? k : 1), *out = NULL, *out2 = NULL; /* exact size: a read past the prefix is reported */
		size_t on = 0, on2 = 0;
		const char *why = NULL;
		memcpy(copy, s, k);
		if (mjh_transcode_memory(copy, (int)k, MJW_OPTIMIZE_HUFFMAN | MJW_COPY_MARKERS, &out, &on, &why)) {
			if (!out || !on) bad++;
		} else if (!why || out) bad++;
		if (mjw_copy_markers(copy, (int)k, s, n, &out2, &on2, &why)) {
			if (!out2 || on2 < n) bad++;
		} else if (!why || out2) bad++;
		free(out); free(out2); free(copy);
	}
	return bad;
}

int main(void)
{
	static const int shapes[5][3] = {{1, 1, 1}, {3, 1, 1}, {3, 2, 1}, {3, 1, 2}, {3, 2, 2}};
	static const int sizes[4][2] = {{1, 1}, {17, 9}, {80, 80}, {131, 67}};
	int si, zi, bad = 0, cases = 0;
	uint32_t seed = 12345u;
	for (si = 0; si < 5; ++si)
		for (zi = 0; zi < 4; ++zi) {
			mij_image_desc d;
			mjw_tplan t;
			const char *why = NULL;
			size_t rbytes, r16bytes = 0, nu, n1, n2;
			uint8_t *r16, *rc;
			int16_t *du, *du2;
			unsigned char *mem, *out = NULL;
			sink a = {0}, b = {0};
			int c;
			make_desc(&d, sizes[zi][0], sizes[zi][1], shapes[si][0], shapes[si][1], shapes[si][2]);
			if (!mjw_tplan_from_desc(&t, &d, &why)) { fprintf(stderr, "shape %d refused: %s\n", si, why); return 1; }
			rbytes = mij_image_region_bytes(&d);
			for (c = 0; c < d.ncomp; ++c)
				r16bytes += mij_plane_elems((uint32_t)(d.comp[c].bw * d.comp[c].bh)) * 2;
			r16 = calloc(1, r16bytes), rc = calloc(1, rbytes);
			for (c = 0; c < d.ncomp; ++c) {
				const uint32_t nblk = (uint32_t)(d.comp[c].bw * d.comp[c].bh);
				uint32_t L;
				int dcv = 0;
				for (L = 0; L < nblk; ++L) {
					const int kind = (int)(lcg(&seed) % 8u);
					int P, nz = kind == 0 ? 0 : kind < 6 ? 5 : 63;
					dcv = (int)(lcg(&seed) % 1001u) - 500; /* |difference| <= 1000 whatever the order */
					put(&d, r16, rc, c, L, 0, dcv);
					for (P = 1; P <= nz; ++P) {
						const int big = kind == 7 || (lcg(&seed) % 16u) == 0;
						const int v = big ? ((lcg(&seed) & 1) ? 1023 : -1023) >> (lcg(&seed) % 3u) : (int)(lcg(&seed) % 61u) - 30;
						put(&d, r16, rc, c, L, kind < 6 ? (int)(lcg(&seed) % 63u) + 1 : P, v);
					}
				}
			}
			nu = mjw_tplan_du_count(&t);
			du = malloc(nu * 128), du2 = malloc(nu * 128);
			if (!mjw_units_from_region(&d, r16, MIJ_COEF_INT16, du) || !mjw_units_from_region(&d, rc, MIJ_COEF_COMPACT, du2) || memcmp(du, du2, nu * 128)) {
				fprintf(stderr, "shape %d size %d: the two plane formats give different units\n", si, zi);
				bad++;
			}
			if (!mjw_tunits_codable(&t, du, &why)) { fprintf(stderr, "shape %d size %d: %s\n", si, zi, why); bad++; }
			mem = malloc(MJW_STREAM_CAP(nu));
			if (!mjw_temit(&t, du, sink_write, &a) || !mjw_temit_optimized(&t, du, sink_write, &b)) bad++;
			n1 = mjw_temit_to_memory(&t, du, 0, mem, MJW_STREAM_CAP(nu));
			if (n1 != a.n || memcmp(mem, a.p, n1)) bad++;
			n2 = mjw_temit_to_memory(&t, du, MJW_OPTIMIZE_HUFFMAN, mem, MJW_STREAM_CAP(nu));
			if (n2 != b.n || memcmp(mem, b.p, n2)) bad++;
			if (mjw_temit_to_memory(&t, du, 0, mem, a.n - 1)) bad++; /* one byte short: refused, nothing written past it */
			if (!mjh_transcode_memory(a.p, (int)a.n, 0, &out, &n1, &why) || n1 != a.n || memcmp(out, a.p, n1)) {
				fprintf(stderr, "shape %d size %d: the plain stream is no fixed point (%s)\n", si, zi, why ? why : "-");
				bad++;
			}
			free(out), out = NULL;
			if (!mjh_transcode_memory(a.p, (int)a.n, MJW_OPTIMIZE_HUFFMAN, &out, &n2, &why) || n2 != b.n || memcmp(out, b.p, n2)) bad++;
			free(out);
			if (zi < 2)
				bad += check_prefixes(b.p, b.n);
			du[64 * (nu - 1) + 63] = 1024; /* one value over: every emitter refuses */
			if (mjw_tunits_codable(&t, du, &why) || mjw_temit(&t, du, sink_write, &a) || mjw_temit_optimized(&t, du, sink_write, &a) ||
				 mjw_temit_to_memory(&t, du, 0, mem, MJW_STREAM_CAP(nu))) bad++;
			free(mem), free(du), free(du2), free(r16), free(rc), free(a.p), free(b.p);
			++cases;
		}
	printf("transcode harness: %d cases, %d failures\n", cases, bad);
	return bad ? 1 : 0;
}
