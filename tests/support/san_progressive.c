/* The progressive writer of the host contract (include/mij_host.h, PROGRESSIVE STREAMS: the mjw_*emit_progressive* calls of
 * image-codecs_amd/csrc/jpeg_write_host.c and the mj?_transcode_memory_progressive* chain) under AddressSanitizer + UBSan, as a stand-alone
 * CPU program (tests/test_progressive_host.py builds and runs it).  For the five MCU shapes and sizes that are no MCU multiple it
 *   - makes units in a heap block of exactly their size: sparse ones, dense ones and runs of empty ones, DC differences and AC values up
 *     to the codable limits, and once enough dense units in a row for the early flush of the correction-bit buffer,
 *   - emits them to a callback and to memory (a buffer of exactly the length, and one byte less, which must fail) and requires both equal,
 *   - walks the stream's segments: SOF2, the scan count of the script, EOI at the end,
 *   - transcodes the stream again with the request (a fixed point), without it and back, and with crop, grey and an orientation,
 *   - and feeds EVERY prefix of one stream to mjh_transcode_memory_progressive.
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

static void make_plan(mjw_tplan *t, int w, int h, int ncomp, int lh, int lv)
{
	int i;
	memset(t, 0, sizeof(*t));
	t->ncomp = ncomp, t->lh = ncomp == 1 ? 1 : lh, t->lv = ncomp == 1 ? 1 : lv;
	t->plan.width = w, t->plan.height = h, t->plan.comp = ncomp, t->plan.subsample = ncomp == 3 && lh == 2 && lv == 2;
	t->plan.mcu_x = (w + 8 * t->lh - 1) / (8 * t->lh), t->plan.mcu_y = (h + 8 * t->lv - 1) / (8 * t->lv);
	t->plan.du_per_mcu = ncomp == 1 ? 1 : t->lh * t->lv + 2;
	for (i = 0; i < 64; ++i)
		t->plan.ytab[i] = (unsigned char)(1 + i % 7), t->plan.ctab[i] = (unsigned char)(ncomp == 1 ? 1 + i % 7 : 255 - i);
}

/* SOF2 present, `want` SOS segments, EOI last: a walk by segment lengths, the entropy-coded bytes skipped up to the next marker */
static int scans_ok(const unsigned char *s, size_t n, int want)
{
	size_t i = 2;
	int sof2 = 0, scans = 0;
	if (n < 4 || s[0] != 0xFF || s[1] != 0xD8 || s[n - 2] != 0xFF || s[n - 1] != 0xD9)
		return 0;
	while (i + 4 <= n) {
		const int m = s[i + 1];
		if (s[i] != 0xFF)
			return 0;
		if (m == 0xD9)
			break;
		sof2 += m == 0xC2;
		i += 2 + ((size_t)s[i + 2] << 8 | s[i + 3]);
		if (m == 0xDA) {
			++scans;
			while (i + 1 < n && !(s[i] == 0xFF && s[i + 1] != 0))
				++i;
		}
	}
	return sof2 == 1 && scans == want && i == n - 2;
}

int main(void)
{
	static const int shapes[5][3] = {{1, 1, 1}, {3, 1, 1}, {3, 2, 1}, {3, 1, 2}, {3, 2, 2}};
	static const int sizes[4][2] = {{1, 1}, {17, 9}, {80, 80}, {131, 67}};
	int si, zi, bad = 0, cases = 0, flushed = 0;
	uint32_t seed = 4711u;
	unsigned char *keep = NULL;
	size_t keep_n = 0;
	for (si = 0; si < 5; ++si)
		for (zi = 0; zi < 4; ++zi) {
			mjw_tplan t;
			mjw_progressive_stats st;
			size_t nu, u, n1, n2;
			int16_t *du;
			unsigned char *mem, *out = NULL, *out2 = NULL;
			const char *why = NULL;
			sink a = {0};
			int k, dc[3] = {0, 0, 0}, ny, rect[4];
			make_plan(&t, sizes[zi][0], sizes[zi][1], shapes[si][0], shapes[si][1], shapes[si][2]);
			nu = mjw_tplan_du_count(&t);
			ny = t.ncomp == 1 ? 1 : t.lh * t.lv;
			du = calloc(nu * 64, sizeof(int16_t)); /* exactly the units: a read past them is reported */
			for (u = 0; u < nu; ++u) {
				const int p = (int)(u % (size_t)t.plan.du_per_mcu), c = p < ny ? 0 : p - ny + 1;
				/* the 80 x 80 grey picture starts with 20 dense units: more than 937 correction bits in a row */
				const int kind = (si == 0 && zi == 2 && u < 20) ? 7 : (int)(lcg(&seed) % 8u);
				int step = (int)(lcg(&seed) % 4095u) - 2047;
				if (dc[c] + step > 2047 || dc[c] + step < -2047)
					step = -dc[c] / 2;
				dc[c] += step;
				du[u * 64] = (int16_t)dc[c];
				if (kind >= 3 && kind < 7) /* sparse: a few coefficients anywhere, small and at the limits */
					for (k = 0; k < 5; ++k) {
						static const int vals[8] = {1, -1, 2, -3, 5, -1023, 1023, 1};
						du[u * 64 + 1 + lcg(&seed) % 63u] = (int16_t)vals[lcg(&seed) % 8u];
					}
				else if (kind == 7) /* dense: no coefficient of magnitude below 2 */
					for (k = 1; k < 64; ++k)
						du[u * 64 + k] = (int16_t)((lcg(&seed) & 1u) ? 2 + (int)(lcg(&seed) % 9u) : -2 - (int)(lcg(&seed) % 9u));
			}
			if (!mjw_tunits_codable(&t, du, &why)) { fprintf(stderr, "case %d/%d: units not codable: %s\n", si, zi, why); return 1; }
			if (!mjw_tprogressive_stats(&t, du, &st)) bad++;
			flushed += st.forced_bit_flushes > 0;
			if (!mjw_temit_progressive(&t, du, sink_write, &a) || !a.n) { fprintf(stderr, "case %d/%d: emit failed\n", si, zi); return 1; }
			if (a.n > MJW_PROGRESSIVE_STREAM_CAP(nu)) bad++;
			mem = malloc(a.n);
			n1 = mjw_temit_progressive_to_memory(&t, du, mem, a.n);
			n2 = a.n > 1 ? mjw_temit_progressive_to_memory(&t, du, mem, a.n - 1) : 0;
			if (n1 != a.n || memcmp(mem, a.p, a.n) || n2 != 0) bad++;
			if (!scans_ok(a.p, a.n, t.ncomp == 1 ? MJW_PROGRESSIVE_SCANS_GREY : MJW_PROGRESSIVE_SCANS_COLOUR)) bad++;
			if (t.ncomp == 3 && t.lh == t.lv) { /* the writer's own two layouts through mjw_emit_progressive */
				sink b = {0};
				if (!mjw_emit_progressive(&t.plan, du, sink_write, &b) || b.n != a.n || memcmp(b.p, a.p, a.n)) bad++;
				n1 = mjw_emit_progressive_to_memory(&t.plan, du, mem, a.n);
				if (n1 != a.n) bad++;
				free(b.p);
			}
			/* the stream transcoded with the request is itself; without it and back again too.  Luma's MCU padding blocks lose their AC
			 * coefficients in the first pass (no AC scan codes them), so the fixed point is judged from the first transcode on. */
			if (!mjh_transcode_memory_progressive(a.p, (int)a.n, 0, 1, 0, NULL, 0, NULL, NULL, 0, 1, &out, &n1, rect, &why)) { fprintf(stderr, "case %d/%d: %s\n", si, zi, why); return 1; }
			if (!mjh_transcode_memory_progressive(out, (int)n1, 0, 1, 0, NULL, 0, NULL, NULL, 0, 1, &out2, &n2, NULL, &why) || n2 != n1 || memcmp(out, out2, n1)) bad++;
			free(out2), out2 = NULL;
			{
				unsigned char *base = NULL;
				size_t nb = 0;
				if (!mjh_transcode_memory_progressive(out, (int)n1, MJW_OPTIMIZE_HUFFMAN, 1, 0, NULL, 0, NULL, NULL, 0, 0, &base, &nb, NULL, &why)) bad++;
				else if (!mjh_transcode_memory_progressive(base, (int)nb, 0, 1, 0, NULL, 0, NULL, NULL, 0, 1, &out2, &n2, NULL, &why) || n2 != n1 || memcmp(out, out2, n1)) bad++;
				free(base), free(out2), out2 = NULL;
			}
			if (mjh_transcode_memory_progressive(out, (int)n1, 0, 1, 0, NULL, 0, NULL, NULL, 0, 2, &out2, &n2, NULL, &why) || out2) bad++; /* not 0 or 1 */
			if (sizes[zi][0] >= 17) { /* crop + grey + transpose with the request */
				const int crop[4] = {1, 1, 7, 6};
				if (!mjh_transcode_memory_progressive(out, (int)n1, MJW_COPY_MARKERS, 5, 0, crop, 1, NULL, NULL, 0, 1, &out2, &n2, rect, &why)) bad++;
				else if (!scans_ok(out2, n2, MJW_PROGRESSIVE_SCANS_GREY)) bad++;
				free(out2), out2 = NULL;
			}
			if (si == 4 && zi == 1) { /* kept for the prefix walk */
				keep = malloc(n1);
				memcpy(keep, out, n1);
				keep_n = n1;
			}
			free(out), free(mem), free(a.p), free(du);
			++cases;
		}
	if (!flushed) { fprintf(stderr, "no case reached the early flush of the correction bits\n"); return 1; }
	{
		size_t k;
		for (k = 0; k < keep_n; ++k) {
			unsigned char *copy = malloc(k ? k : 1), *out = NULL; /* exact size: a read past the prefix is reported */
			size_t on = 0;
			const char *why = NULL;
			memcpy(copy, keep, k);
			if (mjh_transcode_memory_progressive(copy, (int)k, MJW_COPY_MARKERS, 0, 1, NULL, 0, NULL, NULL, 0, 1, &out, &on, NULL, &why)) {
				if (!out || !on) bad++;
			} else if (!why || out) bad++;
			free(out), free(copy);
		}
		free(keep);
	}
	printf("san_progressive: %d cases, %zu prefixes, %d failures\n", cases, keep_n, bad);
	return bad ? 1 : 0;
}
