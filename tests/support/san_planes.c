/* Plane encoding on the host (mjw_pplan_init, mjw_ptransform_host, mjh_write_jpg_planes_to_memory: image-codecs_amd/csrc/jpeg_write_host.c)
 * under AddressSanitizer + UBSan (CPU build only; tests/test_encode_planes_host.py builds and runs this).  Every plane is a heap block of
 * exactly the bytes its (row_pitch, x_pitch) address, and the units a block of exactly mjw_tplan_du_count units, so a read past a plane's
 * last column or row -- the edge rule gone wrong -- or a write past the units is reported:
 *   - the five samplings at sizes around the MCU sizes, planar, with a wider row pitch, as NV12 (x_pitch 2 on one interleaved block, the
 *     Cr plane ending on the block's last byte), flipped, with and without the video-range conversion;
 *   - every transform run twice (equal units) and every stream written plain, optimised, with restarts and progressive.
 * Exit status 0 only when every check held. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "image_api.h"
#include "mij_host.h"

static uint32_t lcg(uint32_t *s) { *s = *s * 1664525u + 1013904223u; return *s >> 8; }
static int bad = 0;
#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); ++bad; } } while (0)

/* a plane of h rows of w samples in an exact-size block: the last sample is the block's last byte */
static unsigned char *plane(int w, int h, int64_t row_pitch, int64_t x_pitch, uint32_t *seed, size_t *bytes)
{
	size_t n = (size_t)((h - 1) * row_pitch + (w - 1) * x_pitch + 1), i;
	unsigned char *p = malloc(n);
	for (i = 0; i < n; ++i)
		p[i] = (unsigned char)lcg(seed);
	*bytes = n;
	return p;
}

static void one(int w, int h, int ncomp, int lh, int lv, int layout, int flip, int vr, uint32_t *seed)
{
	const int cw = (w + lh - 1) / lh, ch = (h + lv - 1) / lv;
	mjw_tplan t;
	mij_plane pl[3];
	mij_in_convert cv;
	unsigned char *blocks[3] = {0, 0, 0};
	size_t n, nu;
	int16_t *du, *du2;
	unsigned char *out;
	size_t out_len;
	int k;
	memset(pl, 0, sizeof pl);
	mjw_video_range(&cv);
	CHECK(mjw_pplan_init(&t, w, h, 75, ncomp, lh, lv, NULL, NULL), "plan %dx%d (%d,%d,%d)", w, h, ncomp, lh, lv);
	blocks[0] = plane(w, h, layout == 1 ? w + 5 : w, 1, seed, &n);
	pl[0] = (mij_plane){blocks[0], layout == 1 ? w + 5 : w, 1};
	if (ncomp == 3 && layout == 2) { /* NV12: one interleaved block; Cr is its odd bytes and ends on its last byte */
		blocks[1] = plane(2 * cw, ch, 2 * cw, 1, seed, &n);
		pl[1] = (mij_plane){blocks[1], 2 * cw, 2};
		pl[2] = (mij_plane){blocks[1] + 1, 2 * cw, 2};
	} else if (ncomp == 3) {
		for (k = 1; k < 3; ++k) {
			blocks[k] = plane(cw, ch, layout == 1 ? cw + 3 : cw, 1, seed, &n);
			pl[k] = (mij_plane){blocks[k], layout == 1 ? cw + 3 : cw, 1};
		}
	}
	nu = mjw_tplan_du_count(&t);
	du = malloc(nu * 128);
	du2 = malloc(nu * 128);
	CHECK(mjw_ptransform_host(&t, pl, vr ? &cv : NULL, flip, du) == 1, "transform %dx%d", w, h);
	CHECK(mjw_ptransform_host(&t, pl, vr ? &cv : NULL, flip, du2) == 1 && !memcmp(du, du2, nu * 128), "transform twice %dx%d", w, h);
	for (k = 0; k < 4; ++k) {
		out = NULL;
		CHECK(mjh_write_jpg_planes_to_memory(pl, w, h, 75, ncomp, lh, lv, NULL, NULL, vr ? &cv : NULL, flip, k == 1 ? MJW_OPTIMIZE_HUFFMAN : 0,
														  k == 2 ? 3 : 0, k == 3, &out, &out_len) == 1 && out && out_len > 4 && out[0] == 0xFF && out[1] == 0xD8 &&
					out[out_len - 2] == 0xFF && out[out_len - 1] == 0xD9,
				"stream %dx%d (%d,%d,%d) form %d", w, h, ncomp, lh, lv, k);
		free(out);
	}
	CHECK(mjh_write_jpg_planes_to_memory(pl, w, h, 75, 0, 0, 0, NULL, NULL, NULL, 0, 0, 0, 0, &out, &out_len) == 0, "a missing sampling is refused");
	free(du);
	free(du2);
	for (k = 0; k < 3; ++k)
		free(blocks[k]);
}

int main(void)
{
	static const int fac[5][3] = {{3, 1, 1}, {3, 2, 1}, {3, 1, 2}, {3, 2, 2}, {1, 1, 1}};
	static const int sizes[6][2] = {{1, 1}, {7, 5}, {8, 8}, {17, 9}, {9, 17}, {33, 31}};
	uint32_t seed = 12345;
	int f, s, layout, n = 0;
	for (f = 0; f < 5; ++f)
		for (s = 0; s < 6; ++s)
			for (layout = 0; layout < 3; ++layout, ++n)
				one(sizes[s][0], sizes[s][1], fac[f][0], fac[f][1], fac[f][2], layout, n & 1, (n >> 1) & 1, &seed);
	printf("planes harness: %d cases, %d failures\n", n, bad);
	return bad != 0;
}
