/* The host half of the lossless reorientation (mjw_tplan_oriented, mjw_units_orient, mjh_transcode_memory_oriented,
 * mjh_exif_set_orientation) under AddressSanitizer + UBSan, as a stand-alone CPU program (tests/test_transcode_orient_host.py builds and
 * runs it).  For the five MCU shapes and sizes that are and are not MCU multiples, every orientation 0..9 and both edge modes, it
 *   - makes the destination plan and converts random units between heap blocks of exactly the source's and the destination's sizes,
 *   - requires o followed by its inverse to give the source's units back where nothing was trimmed, and o = 1 to be a copy,
 *   - emits the source, puts an Exif APP1 (either byte order) behind its SOI, and runs the whole-file call on it with copied markers:
 *     the result's tag must read 1, and orientation 0 must equal the explicit orientation of the tag,
 *   - runs mjh_exif_set_orientation and the whole-file call on EVERY prefix of the tagged header, in blocks of exactly the prefix's size.
 * Exit status 0 only when every comparison held. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mij_host.h"

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

/* `stream` with an Exif APP1 of the given orientation behind SOI, in a block of exactly its size */
static unsigned char *tagged(const unsigned char *stream, size_t n, int le, int value, size_t *out_n)
{
	static const unsigned char ii[] = {0xFF, 0xE1, 0, 34, 'E', 'x', 'i', 'f', 0, 0, 'I', 'I', 42, 0, 8, 0, 0, 0, 1, 0, 0x12, 0x01, 3, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	static const unsigned char mm[] = {0xFF, 0xE1, 0, 34, 'E', 'x', 'i', 'f', 0, 0, 'M', 'M', 0, 42, 0, 0, 0, 8, 0, 1, 0x01, 0x12, 0, 3, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0};
	unsigned char *p = malloc(n + sizeof(ii));
	memcpy(p, stream, 2);
	memcpy(p + 2, le ? ii : mm, sizeof(ii));
	p[2 + (le ? 28 : 29)] = (unsigned char)value;
	memcpy(p + 2 + sizeof(ii), stream + 2, n - 2);
	*out_n = n + sizeof(ii);
	return p;
}

int main(void)
{
	static const int shapes[5][3] = {{1, 1, 1}, {3, 1, 1}, {3, 2, 1}, {3, 1, 2}, {3, 2, 2}};
	static const int sizes[4][2] = {{5, 3}, {32, 48}, {45, 32}, {83, 51}};
	static const int inverse[9] = {0, 1, 2, 3, 4, 5, 8, 7, 6};
	int si, zi, o, trim, bad = 0, cases = 0;
	uint32_t seed = 2024u;
	for (si = 0; si < 5; ++si)
		for (zi = 0; zi < 4; ++zi) {
			mij_image_desc d;
			mjw_tplan t, dt, back;
			const char *why = NULL;
			size_t nu, i, n, tn;
			int16_t *du;
			unsigned char *mem, *tag;
			make_desc(&d, sizes[zi][0], sizes[zi][1], shapes[si][0], shapes[si][1], shapes[si][2]);
			if (!mjw_tplan_from_desc(&t, &d, &why)) { fprintf(stderr, "shape %d refused: %s\n", si, why); return 1; }
			nu = mjw_tplan_du_count(&t);
			du = malloc(nu * 128);
			for (i = 0; i < nu * 64; ++i)
				du[i] = (int16_t)((i % 64) ? ((lcg(&seed) % 5u) ? 0 : (int)(lcg(&seed) % 2047u) - 1023) : (int)(lcg(&seed) % 1001u) - 500);
			for (o = -1; o <= 9; ++o)
				for (trim = 0; trim < 2; ++trim) {
					int16_t *dd, *bk;
					size_t dn;
					why = NULL;
					if (!mjw_tplan_oriented(&dt, &t, o, trim, &why)) {
						int16_t none[1];
						if (!why || mjw_units_orient(&t, du, o, trim, none)) bad++; /* refused: nothing may be written */
						continue;
					}
					if (o < 1 || o > 8) { bad++; continue; }
					dn = mjw_tplan_du_count(&dt);
					dd = malloc(dn * 128);
					if (!mjw_units_orient(&t, du, o, trim, dd)) bad++;
					if (o == 1 && (dn != nu || memcmp(dd, du, nu * 128) || memcmp(&dt, &t, sizeof(t)))) bad++;
					if (!mjw_tunits_codable(&dt, dd, &why)) bad++; /* DCs within +-500: codable in any order */
					if (dn == nu && mjw_tplan_oriented(&back, &dt, inverse[o], 0, &why)) { /* nothing trimmed, and the way back is perfect */
						bk = malloc(nu * 128);
						if (!mjw_units_orient(&dt, dd, inverse[o], 0, bk) || memcmp(bk, du, nu * 128) || memcmp(&back, &t, sizeof(t))) {
							fprintf(stderr, "shape %d size %d o %d: the inverse does not give the source back\n", si, zi, o);
							bad++;
						}
						free(bk);
					}
					free(dd);
				}
			/* whole files */
			mem = malloc(MJW_STREAM_CAP(nu));
			n = mjw_temit_to_memory(&t, du, MJW_OPTIMIZE_HUFFMAN, mem, MJW_STREAM_CAP(nu));
			if (!n) { fprintf(stderr, "shape %d size %d: no stream\n", si, zi); return 1; }
			for (o = 1; o <= 8; ++o) {
				const int le = o & 1;
				unsigned char *a = NULL, *b = NULL;
				size_t an = 0, bn = 0;
				int oka, okb;
				tag = tagged(mem, n, le, o, &tn);
				if (mjh_exif_orientation(tag, (int)tn) != o) bad++;
				for (trim = 0; trim < 2; ++trim) {
					oka = mjh_transcode_memory_oriented(tag, (int)tn, MJW_COPY_MARKERS, 0, trim, &a, &an, &why);
					okb = mjh_transcode_memory_oriented(tag, (int)tn, MJW_COPY_MARKERS, o, trim, &b, &bn, &why);
					if (oka != okb || (oka && (an != bn || memcmp(a, b, an) || mjh_exif_orientation(a, (int)an) != 1))) {
						fprintf(stderr, "shape %d size %d o %d trim %d: the tag's orientation and the explicit one differ\n", si, zi, o, trim);
						bad++;
					}
					if (!oka && (a || !why)) bad++;
					free(a), free(b), a = b = NULL;
				}
				if (zi == 0 || (zi == 2 && o == 6)) { /* every prefix of the tagged header, and a few longer ones */
					size_t k;
					for (k = 0; k <= tn; k += (k < 80 || tn - k < 8) ? 1 : 29) {
						unsigned char *copy = malloc(k ? k : 1), *out = NULL;
						size_t on = 0;
						memcpy(copy, tag, k);
						if (mjh_exif_set_orientation(copy, (int)k, 1) != (k >= 38)) bad++; /* SOI and the whole 36-byte APP1 must be there */
						if (mjh_transcode_memory_oriented(copy, (int)k, MJW_COPY_MARKERS | MJW_OPTIMIZE_HUFFMAN, 0, 1, &out, &on, &why)) {
							if (!out || !on) bad++;
						} else if (!why || out) bad++;
						free(out), free(copy);
					}
				}
				free(tag);
			}
			free(mem), free(du);
			++cases;
		}
	printf("orientation harness: %d cases, %d failures\n", cases, bad);
	return bad ? 1 : 0;
}
