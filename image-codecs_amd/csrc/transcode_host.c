/*
 * transcode_host.c -- the host half of the lossless transcode (include/mij_host.h, mjw_tplan): which sources are transcodable, the
 * coefficient planes read as the writer's data units, the orientation, requantisation, greyscale and crop steps, the marker copy, and
 * the whole path on the host (mjh_transcode_memory, mjw_transcode_memory_window_at).  The
 * emission itself is the writer's (jpeg_write_host.c: mjw_temit).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mij_host.h"

/* natural index -> zigzag position (codec/jpeg_write.c:1-2) */
static const unsigned char k_zigzag_of[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
															 41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
															 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

static int refuse(const char **reason, const char *why)
{
	if (reason)
		*reason = why;
	return 0;
}

int mjw_tplan_from_desc(mjw_tplan *t, const mij_image_desc *d, const char **reason)
{
	int c, i;
	if (!t || !d)
		return refuse(reason, "bad argument");
	if (d->width <= 0 || d->height <= 0 || d->width > 65535 || d->height > 65535 || d->mcu_x <= 0 || d->mcu_y <= 0)
		return refuse(reason, "bad picture size");
	if (d->ncomp == 4)
		return refuse(reason, "four-component (CMYK / YCCK) source");
	if (d->ncomp != 1 && d->ncomp != 3)
		return refuse(reason, "component count not 1 or 3");
	if (d->ncomp == 3 && d->color == MIJ_COLOR_RGB)
		return refuse(reason, "RGB-tagged source");
	if (d->ncomp == 3 && d->color != MIJ_COLOR_YCBCR)
		return refuse(reason, "colour mode is not YCbCr");
	for (c = 1; c < d->ncomp; ++c)
		if (d->comp[c].h != 1 || d->comp[c].v != 1)
			return refuse(reason, "chroma sampling factors other than 1x1");
	if (d->ncomp == 1 && (d->comp[0].h != 1 || d->comp[0].v != 1))
		return refuse(reason, "grey sampling factors other than 1x1");
	if (d->comp[0].h < 1 || d->comp[0].h > 2 || d->comp[0].v < 1 || d->comp[0].v > 2)
		return refuse(reason, "luma sampling factors beyond 2x2 (4:1:1 and the like)");
	for (c = 0; c < d->ncomp; ++c) {
		if (d->comp[c].tq < 0 || d->comp[c].tq > 3)
			return refuse(reason, "bad quantisation table index");
		if (d->comp[c].bw != d->mcu_x * d->comp[c].h || d->comp[c].bh != d->mcu_y * d->comp[c].v)
			return refuse(reason, "block grid does not match the MCU grid");
		for (i = 0; i < 64; ++i)
			if (d->dequant[d->comp[c].tq][i] > 255 || d->dequant[d->comp[c].tq][i] < 1)
				return refuse(reason, "a quantisation table entry outside 1..255 (16-bit tables are not written)");
	}
	if (d->ncomp == 3 && memcmp(d->dequant[d->comp[1].tq], d->dequant[d->comp[2].tq], sizeof(d->dequant[0])))
		return refuse(reason, "Cb and Cr use different quantisation tables");
	memset(t, 0, sizeof(*t));
	t->ncomp = d->ncomp;
	t->lh = d->comp[0].h;
	t->lv = d->comp[0].v;
	t->plan.width = d->width;
	t->plan.height = d->height;
	t->plan.comp = d->ncomp;
	t->plan.subsample = t->lh == 2 && t->lv == 2;
	t->plan.mcu_x = d->mcu_x;
	t->plan.mcu_y = d->mcu_y;
	t->plan.du_per_mcu = d->ncomp == 1 ? 1 : t->lh * t->lv + 2;
	for (i = 0; i < 64; ++i) {
		t->plan.ytab[k_zigzag_of[i]] = (unsigned char)d->dequant[d->comp[0].tq][i];
		t->plan.ctab[k_zigzag_of[i]] = (unsigned char)d->dequant[d->comp[d->ncomp == 3 ? 1 : 0].tq][i];
	}
	if ((size_t)d->mcu_x * (size_t)d->mcu_y > ((size_t)1 << 26))
		return refuse(reason, "too many MCUs");
	return 1;
}

/* coefficient at in-block position P of block L of a component, in either plane format */
typedef struct {
	const int16_t *plane;               /* int16 tile layout */
	const uint8_t *lo, *hi, *dc;        /* compact planes */
} comp_src;

static void read_block(const comp_src *s, int compact, size_t L, int16_t *du)
{
	int k;
	if (!compact) {
		for (k = 0; k < 64; ++k)
			du[k] = s->plane[mij_coef_index((uint32_t)L, mij_zigzag_pos[k])];
		return;
	}
	{
		const uint8_t *blo = s->lo + ((L >> 6) << 12) + ((L & 63) << 3);
		const int esc = blo[0] & 1;
		uint16_t dcv;
		for (k = 1; k < 64; ++k) {
			const int P = mij_zigzag_pos[k];
			int v = (int8_t)blo[((size_t)(P >> 3) << 9) + (P & 7)];
			if (esc)
				v += 256 * (int)(int8_t)s->hi[(L << 6) + (size_t)P];
			du[k] = (int16_t)v;
		}
		memcpy(&dcv, s->dc + 2 * L, 2);
		du[0] = (int16_t)dcv;
	}
}

int mjw_units_from_region(const mij_image_desc *d, const uint8_t *region, int format, int16_t *du)
{
	mjw_tplan t;
	comp_src src[3];
	size_t off = 0;
	int c, mx, my, sx, sy;
	if (!region || !du || (format != MIJ_COEF_INT16 && format != MIJ_COEF_COMPACT) || !mjw_tplan_from_desc(&t, d, NULL))
		return 0;
	for (c = 0; c < d->ncomp; ++c) {
		memset(&src[c], 0, sizeof(src[c]));
		if (format == MIJ_COEF_COMPACT) {
			size_t lo, dc, hi;
			mij_compact_offsets(d, c, &lo, &dc, &hi);
			src[c].lo = region + lo;
			src[c].dc = region + dc;
			src[c].hi = region + hi;
		} else {
			src[c].plane = (const int16_t *)(const void *)(region + off);
			off += mij_plane_elems((uint32_t)(d->comp[c].bw * d->comp[c].bh)) * sizeof(int16_t);
		}
	}
	for (my = 0; my < d->mcu_y; ++my)
		for (mx = 0; mx < d->mcu_x; ++mx)
			for (c = 0; c < d->ncomp; ++c) {
				const mij_comp_desc *cp = &d->comp[c];
				for (sy = 0; sy < cp->v; ++sy)
					for (sx = 0; sx < cp->h; ++sx, du += 64)
						read_block(&src[c], format == MIJ_COEF_COMPACT, (size_t)(mx * cp->h + sx) + (size_t)(my * cp->v + sy) * (size_t)cp->bw, du);
			}
	return 1;
}

/* ---- orientation (mjw_tplan_oriented, include/mij_host.h): mirrors of the source's axes first, then an optional transpose */
static const unsigned char k_orient_tr[9] = {0, 0, 0, 0, 0, 1, 1, 1, 1}, k_orient_mx[9] = {0, 0, 1, 1, 0, 0, 0, 1, 1},
									k_orient_my[9] = {0, 0, 0, 1, 1, 0, 1, 1, 0};

/* one mirrored axis: its size in pixels and MCUs after the edge mode; 0 with *reason where the picture is refused */
static int mirror_axis(const char *axis, const char *name, int *size, int *mcus, int mcu_px, int trim, const char **reason)
{
	static _Thread_local char why[2][160]; /* one per axis; static strings as every other reason is */
	char *w = why[axis[0] == 'y'];
	if (*size % mcu_px == 0)
		return 1;
	if (!trim) {
		snprintf(w, sizeof(why[0]), "not perfect: the mirrored %s axis (%s %d) is no multiple of the MCU size %d; edge mode trim drops the partial MCU", axis,
					name, *size, mcu_px);
		return refuse(reason, w);
	}
	if (*size < mcu_px) {
		snprintf(w, sizeof(why[0]), "nothing left after the trim: the mirrored %s axis (%s %d) is smaller than the MCU size %d", axis, name, *size, mcu_px);
		return refuse(reason, w);
	}
	*mcus = *size / mcu_px;
	*size = *mcus * mcu_px;
	return 1;
}

int mjw_tplan_oriented(mjw_tplan *dst, const mjw_tplan *src, int o, int trim, const char **reason)
{
	mjw_tplan t;
	int w, h, ex, ey, r, c;
	if (!dst || !src)
		return refuse(reason, "bad argument");
	if (o < 1 || o > 8)
		return refuse(reason, "orientation is not 1..8");
	if (src->lh < 1 || src->lh > 2 || src->lv < 1 || src->lv > 2 || src->plan.mcu_x < 1 || src->plan.mcu_y < 1)
		return refuse(reason, "bad source plan");
	t = *src;
	w = src->plan.width, h = src->plan.height, ex = src->plan.mcu_x, ey = src->plan.mcu_y;
	if (k_orient_mx[o] && !mirror_axis("x", "width", &w, &ex, 8 * src->lh, trim, reason))
		return 0;
	if (k_orient_my[o] && !mirror_axis("y", "height", &h, &ey, 8 * src->lv, trim, reason))
		return 0;
	if (!k_orient_tr[o]) {
		t.plan.width = w, t.plan.height = h, t.plan.mcu_x = ex, t.plan.mcu_y = ey;
	} else {
		t.plan.width = h, t.plan.height = w, t.plan.mcu_x = ey, t.plan.mcu_y = ex;
		t.lh = src->lv, t.lv = src->lh;
		for (r = 0; r < 8; ++r)
			for (c = 0; c < 8; ++c) {
				t.plan.ytab[k_zigzag_of[8 * r + c]] = src->plan.ytab[k_zigzag_of[8 * c + r]];
				t.plan.ctab[k_zigzag_of[8 * r + c]] = src->plan.ctab[k_zigzag_of[8 * c + r]];
			}
	}
	*dst = t;
	return 1;
}

int mjw_units_orient(const mjw_tplan *src, const int16_t *du_src, int o, int trim, int16_t *du_dst)
{
	mjw_tplan t;
	unsigned char from[64], neg[64];
	int r, c, k, comp, mx, my, sx, sy;
	if (!du_src || !du_dst || !mjw_tplan_oriented(&t, src, o, trim, NULL))
		return 0;
	{
		const int tr = k_orient_tr[o], fx = k_orient_mx[o], fy = k_orient_my[o];
		const int ny = src->ncomp == 1 ? 1 : src->lh * src->lv, dpm = src->plan.du_per_mcu;
		/* the source's MCUs that stay: the destination's, swapped back */
		const int ex = tr ? t.plan.mcu_y : t.plan.mcu_x, ey = tr ? t.plan.mcu_x : t.plan.mcu_y;
		for (r = 0; r < 8; ++r) /* destination (v = r, u = c) takes source (v, u) = (c, r) when transposed; odd source u / v change sign */
			for (c = 0; c < 8; ++c) {
				const int sr = tr ? c : r, sc = tr ? r : c;
				from[k_zigzag_of[8 * r + c]] = k_zigzag_of[8 * sr + sc];
				neg[k_zigzag_of[8 * r + c]] = (unsigned char)(((fx && (sc & 1)) ? 1 : 0) ^ ((fy && (sr & 1)) ? 1 : 0));
			}
		for (my = 0; my < t.plan.mcu_y; ++my)
			for (mx = 0; mx < t.plan.mcu_x; ++mx)
				for (comp = 0; comp < t.ncomp; ++comp) {
					const int dh = comp ? 1 : t.lh, dv = comp ? 1 : t.lv, sh = comp ? 1 : src->lh, sv = comp ? 1 : src->lv;
					for (sy = 0; sy < dv; ++sy)
						for (sx = 0; sx < dh; ++sx, du_dst += 64) {
							const int dbx = mx * dh + sx, dby = my * dv + sy;
							int bx = tr ? dby : dbx, by = tr ? dbx : dby;
							const int16_t *s;
							if (fx)
								bx = ex * sh - 1 - bx;
							if (fy)
								by = ey * sv - 1 - by;
							s = du_src + 64 * (((size_t)(by / sv) * (size_t)src->plan.mcu_x + (size_t)(bx / sh)) * (size_t)dpm +
													 (size_t)(comp ? ny + comp - 1 : (by % sv) * sh + bx % sh));
							for (k = 0; k < 64; ++k)
								du_dst[k] = neg[k] ? (int16_t)-s[from[k]] : s[from[k]];
						}
				}
	}
	return 1;
}

/* ---- requantisation (mjw_tplan_requant, include/mij_host.h): new tables in the coefficient domain, after the orientation */
int mjw_tplan_requant(mjw_tplan *dst, const mjw_tplan *src, const unsigned char luma[64], const unsigned char chroma[64], int coarsen_only,
                      const char **reason)
{
	mjw_tplan t;
	int k, changed = 0;
	if (!dst || !src || !luma || !chroma)
		return refuse(reason, "bad argument");
	t = *src;
	for (k = 0; k < 64; ++k) {
		if (!luma[k] || !chroma[k] || !src->plan.ytab[k] || !src->plan.ctab[k])
			return refuse(reason, "a quantisation table entry of zero");
		t.plan.ytab[k] = coarsen_only && src->plan.ytab[k] > luma[k] ? src->plan.ytab[k] : luma[k];
		if (src->ncomp == 3)
			t.plan.ctab[k] = coarsen_only && src->plan.ctab[k] > chroma[k] ? src->plan.ctab[k] : chroma[k];
		else /* grey: one table, kept in both places as mjw_tplan_from_desc leaves it */
			t.plan.ctab[k] = t.plan.ytab[k];
		changed |= t.plan.ytab[k] != src->plan.ytab[k] || t.plan.ctab[k] != src->plan.ctab[k];
	}
	*dst = t;
	return changed ? 2 : 1;
}

uint32_t mjw_requant_magic(int b, uint32_t *inc)
{
	if (inc)
		*inc = b == 1;
	if (b < 1 || b > 255)
		return 0u;
	return b == 1 ? 0xFFFFFFFFu : (uint32_t)(((uint64_t)1 << 32) / (uint32_t)b) + 1u;
}

int mjw_units_requant(const mjw_tplan *src, const mjw_tplan *dst, const int16_t *du_src, int16_t *du_dst)
{
	size_t u, nu;
	int k, ny, dpm;
	if (!src || !dst || !du_src || !du_dst || src->ncomp != dst->ncomp || src->plan.du_per_mcu != dst->plan.du_per_mcu || src->plan.du_per_mcu < 1 ||
		 mjw_tplan_du_count(src) != mjw_tplan_du_count(dst))
		return 0;
	for (k = 0; k < 64; ++k)
		if (!dst->plan.ytab[k] || (dst->ncomp == 3 && !dst->plan.ctab[k]))
			return 0;
	nu = mjw_tplan_du_count(src);
	dpm = src->plan.du_per_mcu;
	ny = src->ncomp == 1 ? 1 : dpm - 2;
	for (u = 0; u < nu; ++u, du_src += 64, du_dst += 64) {
		const int chroma = (int)(u % (size_t)dpm) >= ny;
		const unsigned char *a = chroma ? src->plan.ctab : src->plan.ytab, *b = chroma ? dst->plan.ctab : dst->plan.ytab;
		for (k = 0; k < 64; ++k) {
			const int x = du_src[k] * a[k], m = ((x < 0 ? -x : x) + (b[k] >> 1)) / b[k];
			du_dst[k] = (int16_t)(m > 32767 ? (x < 0 ? -32767 : 32767) : (x < 0 ? -m : m));
		}
	}
	return 1;
}

int mjw_copy_markers(const uint8_t *src, int src_len, const unsigned char *stream, size_t stream_len, unsigned char **out, size_t *out_len,
                     const char **reason)
{
	static const size_t own = 18; /* the writer's APP0 behind SOI */
	size_t copy = 0, o;
	int i, pass, has_own = 0;
	unsigned char *dst = NULL;
	if (!out || !out_len)
		return refuse(reason, "bad argument");
	*out = NULL;
	*out_len = 0;
	if (!src || src_len < 4 || src[0] != 0xFF || src[1] != 0xD8)
		return refuse(reason, "source has no SOI");
	if (!stream || stream_len < 2 + own || stream[2] != 0xFF || stream[3] != 0xE0)
		return refuse(reason, "stream does not start with SOI and APP0");
	for (pass = 0; pass < 2; ++pass) { /* measure, then copy */
		o = 2;
		if (pass) {
			dst = (unsigned char *)malloc(stream_len + copy);
			if (!dst)
				return refuse(reason, "out of memory");
			dst[0] = 0xFF;
			dst[1] = 0xD8;
			if (!has_own) {
				memcpy(dst + o, stream + 2, own);
				o += own;
			}
		}
		for (i = 2;;) {
			int m, n;
			if (i + 2 > src_len)
				return free(dst), refuse(reason, "source ends before its first SOS");
			if (src[i] != 0xFF)
				return free(dst), refuse(reason, "source has bytes that are no marker in front of its first SOS");
			m = src[i + 1];
			if (m == 0xFF) { /* fill byte */
				++i;
				continue;
			}
			if (m == 0xDA)
				break;
			if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) {
				i += 2;
				continue;
			}
			if (m == 0xD9 || m == 0x00)
				return free(dst), refuse(reason, "source ends before its first SOS");
			if (i + 4 > src_len)
				return free(dst), refuse(reason, "a segment length is cut off");
			n = (src[i + 2] << 8) | src[i + 3];
			if (n < 2 || i + 2 + n > src_len)
				return free(dst), refuse(reason, "a segment length runs past the end of the source");
			if ((m >= 0xE0 && m <= 0xEF) || m == 0xFE) {
				if (!pass) {
					copy += (size_t)n + 2;
					if ((m == 0xE0 && n >= 7 && !memcmp(src + i + 4, "JFIF", 5)) || (m == 0xEE && n >= 7 && !memcmp(src + i + 4, "Adobe", 5)))
						has_own = 1;
				} else {
					memcpy(dst + o, src + i, (size_t)n + 2);
					o += (size_t)n + 2;
				}
			}
			i += 2 + n;
		}
	}
	memcpy(dst + o, stream + 2 + own, stream_len - 2 - own);
	o += stream_len - 2 - own;
	*out = dst;
	*out_len = o;
	return 1;
}

/* ---- greyscale and crop (mjw_tplan_grey, mjw_tplan_cropped, include/mij_host.h): which blocks go where, no coefficient value changes;
 * and the whole chain grey -> orient -> crop -> requantise -> emit, which needs no EXIF code (mjh_transcode_memory_window,
 * transcode_orient.c, adds the file's tag) */
static int plan_ok(const mjw_tplan *t)
{
	return t && (t->ncomp == 1 || t->ncomp == 3) && t->lh >= 1 && t->lh <= 2 && t->lv >= 1 && t->lv <= 2 && t->plan.mcu_x >= 1 && t->plan.mcu_y >= 1 &&
			 t->plan.width >= 1 && t->plan.height >= 1 && t->plan.du_per_mcu == (t->ncomp == 1 ? 1 : t->lh * t->lv + 2) && (t->ncomp == 3 || (t->lh == 1 && t->lv == 1));
}

int mjw_tplan_grey(mjw_tplan *dst, const mjw_tplan *src)
{
	mjw_tplan t;
	if (!dst || !plan_ok(src))
		return 0;
	t = *src;
	if (src->ncomp == 3) {
		t.ncomp = 1;
		t.lh = t.lv = 1;
		t.plan.comp = 1;
		t.plan.subsample = 0;
		t.plan.mcu_x = (src->plan.width + 7) / 8;
		t.plan.mcu_y = (src->plan.height + 7) / 8;
		t.plan.du_per_mcu = 1;
		memcpy(t.plan.ctab, t.plan.ytab, sizeof(t.plan.ctab));
	}
	*dst = t;
	return 1;
}

int mjw_units_grey(const mjw_tplan *src, const int16_t *du_src, int16_t *du_dst)
{
	mjw_tplan t;
	int bx, by;
	if (!du_src || !du_dst || !mjw_tplan_grey(&t, src))
		return 0;
	if (src->ncomp == 1) {
		memcpy(du_dst, du_src, mjw_tplan_du_count(src) * 64 * sizeof(int16_t));
		return 1;
	}
	for (by = 0; by < t.plan.mcu_y; ++by)
		for (bx = 0; bx < t.plan.mcu_x; ++bx, du_dst += 64)
			memcpy(du_dst,
					 du_src + 64 * (((size_t)(by / src->lv) * (size_t)src->plan.mcu_x + (size_t)(bx / src->lh)) * (size_t)src->plan.du_per_mcu +
										 (size_t)((by % src->lv) * src->lh + bx % src->lh)),
					 64 * sizeof(int16_t));
	return 1;
}

int mjw_tplan_cropped(mjw_tplan *dst, const mjw_tplan *src, int x0, int y0, int w, int h, int rect[4], const char **reason)
{
	static _Thread_local char why[200];
	mjw_tplan t;
	int mw, mh, dx, dy;
	if (!dst || !plan_ok(src))
		return refuse(reason, "bad argument");
	if (w < 1 || h < 1 || x0 < 0 || y0 < 0 || x0 > src->plan.width - w || y0 > src->plan.height - h) {
		snprintf(why, sizeof(why), "the window %dx%d+%d+%d does not lie inside the picture (%d x %d)", w, h, x0, y0, src->plan.width, src->plan.height);
		return refuse(reason, why);
	}
	mw = 8 * src->lh, mh = 8 * src->lv;
	dx = x0 % mw, dy = y0 % mh;
	t = *src;
	t.plan.width = w + dx;
	t.plan.height = h + dy;
	t.plan.mcu_x = (t.plan.width + mw - 1) / mw;
	t.plan.mcu_y = (t.plan.height + mh - 1) / mh;
	if (rect)
		rect[0] = x0 - dx, rect[1] = y0 - dy, rect[2] = t.plan.width, rect[3] = t.plan.height;
	*dst = t;
	return 1;
}

int mjw_units_crop(const mjw_tplan *src, const int16_t *du_src, const int rect[4], int16_t *du_dst)
{
	mjw_tplan t;
	int my, kept[4];
	if (!du_src || !du_dst || !rect || !mjw_tplan_cropped(&t, src, rect[0], rect[1], rect[2], rect[3], kept, NULL) || kept[0] != rect[0] || kept[1] != rect[1])
		return 0; /* rect is a kept rectangle: its origin lies on the MCU grid */
	{
		const size_t row = (size_t)t.plan.mcu_x * (size_t)src->plan.du_per_mcu * 64;
		const int mx0 = rect[0] / (8 * src->lh), my0 = rect[1] / (8 * src->lv);
		for (my = 0; my < t.plan.mcu_y; ++my)
			memcpy(du_dst + (size_t)my * row,
					 du_src + ((size_t)(my + my0) * (size_t)src->plan.mcu_x + (size_t)mx0) * (size_t)src->plan.du_per_mcu * 64, row * sizeof(int16_t));
	}
	return 1;
}

/* one step's units replace the previous step's */
static int16_t *units_for(const mjw_tplan *t) { return (int16_t *)malloc(mjw_tplan_du_count(t) * 64 * sizeof(int16_t)); }

/* the whole chain; progressive 1 ends it in mjw_temit_progressive (include/mij_host.h, PROGRESSIVE STREAMS), which takes no interval */
static int transcode_memory_at(const uint8_t *src, int len, unsigned flags, int o, int trim, const int *crop, int grey, const unsigned char *luma,
                               const unsigned char *chroma, int coarsen_only, int restart_rows, int restart_mcus, int progressive, unsigned char **out,
                               size_t *out_len, int *rect_out, int *ri_out, const char **reason)
{
	mij_image_desc d;
	int ri = 0;
	mjw_tplan t, next;
	const char *why = NULL;
	uint8_t *region = NULL;
	int16_t *du = NULL, *dn = NULL;
	unsigned char *buf = NULL;
	size_t rbytes, cap, n = 0;
	int ok = 0, rect[4];
	if (!out || !out_len)
		return refuse(reason, "bad argument");
	*out = NULL;
	*out_len = 0;
	if (!src || len <= 0 || !luma != !chroma)
		return refuse(reason, "bad argument");
	if (flags & ~(MJW_OPTIMIZE_HUFFMAN | MJW_COPY_MARKERS))
		return refuse(reason, "unknown flag");
	if (progressive != 0 && progressive != 1)
		return refuse(reason, "progressive is 0 or 1");
	if (progressive && (restart_rows || restart_mcus))
		return refuse(reason, "restart intervals are not combined with progressive output");
	if (!mjh_probe_memory(src, len, 0, &d, &why))
		return refuse(reason, why ? why : "decode failed");
	rbytes = mij_image_region_bytes(&d);
	region = (uint8_t *)malloc(rbytes ? rbytes : 1);
	if (!region)
		return refuse(reason, "out of memory");
	if (!mjh_decode_memory_fmt(src, len, 0, &d, region, rbytes, 0, &why)) {
		refuse(reason, why ? why : "decode failed");
		goto done;
	}
	if (!mjw_tplan_from_desc(&t, &d, reason))
		goto done;
	du = units_for(&t);
	if (!du) {
		refuse(reason, "out of memory");
		goto done;
	}
	if (!mjw_units_from_region(&d, region, (d.flags & MIJ_FLAG_STAGED_COMPACT) ? MIJ_COEF_COMPACT : MIJ_COEF_INT16, du)) {
		refuse(reason, "units could not be read");
		goto done;
	}
#define STEP(plan_call, units_call)            \
	do {                                        \
		if (!(plan_call))                        \
			goto done;                            \
		dn = units_for(&next);                   \
		if (!dn || !(units_call)) {              \
			refuse(reason, dn ? "units could not be read" : "out of memory"); \
			goto done;                            \
		}                                        \
		free(du);                                \
		du = dn, dn = NULL, t = next;            \
	} while (0)
	if (grey && t.ncomp == 3)
		STEP(mjw_tplan_grey(&next, &t) || refuse(reason, "bad source plan"), mjw_units_grey(&t, du, dn));
	if (o != 1)
		STEP(mjw_tplan_oriented(&next, &t, o, trim, reason), mjw_units_orient(&t, du, o, trim, dn));
	else if (!mjw_tplan_oriented(&next, &t, o, trim, reason))
		goto done;
	rect[0] = rect[1] = 0, rect[2] = t.plan.width, rect[3] = t.plan.height;
	if (crop)
		STEP(mjw_tplan_cropped(&next, &t, crop[0], crop[1], crop[2], crop[3], rect, reason), mjw_units_crop(&t, du, rect, dn));
	if (luma) { /* a plan whose tables did not change keeps its units */
		const int rq = mjw_tplan_requant(&next, &t, luma, chroma, coarsen_only, reason);
		if (!rq)
			goto done;
		if (rq == 2)
			STEP(1, mjw_units_requant(&t, &next, du, dn));
	}
#undef STEP
	/* the interval is one of the destination: its MCU rows are the rows after grey, orientation and crop */
	if (!mjw_restart_interval(&t, restart_rows, restart_mcus, &ri, reason))
		goto done;
	if (!mjw_tunits_codable_restart(&t, du, ri, reason))
		goto done;
	cap = progressive ? MJW_PROGRESSIVE_STREAM_CAP(mjw_tplan_du_count(&t)) : MJW_STREAM_CAP(mjw_tplan_du_count(&t));
	buf = (unsigned char *)malloc(cap);
	if (!buf) {
		refuse(reason, "out of memory");
		goto done;
	}
	n = progressive ? mjw_temit_progressive_to_memory(&t, du, buf, cap) : ri ? mjw_temit_restart_to_memory(&t, du, flags & MJW_OPTIMIZE_HUFFMAN, ri, buf, cap) : mjw_temit_to_memory(&t, du, flags & MJW_OPTIMIZE_HUFFMAN, buf, cap);
	if (!n) {
		refuse(reason, "emission failed");
		goto done;
	}
	if (flags & MJW_COPY_MARKERS) {
		ok = mjw_copy_markers(src, len, buf, n, out, out_len, reason);
	} else {
		*out = buf;
		*out_len = n;
		buf = NULL;
		ok = 1;
	}
	if (ok && rect_out)
		memcpy(rect_out, rect, sizeof(rect));
	if (ok && ri_out)
		*ri_out = ri;
done:
	free(region);
	free(du);
	free(dn);
	free(buf);
	return ok;
}

int mjw_transcode_memory_restart_at(const uint8_t *src, int len, unsigned flags, int o, int trim, const int *crop, int grey, const unsigned char *luma,
                                    const unsigned char *chroma, int coarsen_only, int restart_rows, int restart_mcus, unsigned char **out,
                                    size_t *out_len, int *rect_out, int *ri_out, const char **reason)
{
	return transcode_memory_at(src, len, flags, o, trim, crop, grey, luma, chroma, coarsen_only, restart_rows, restart_mcus, 0, out, out_len, rect_out,
										ri_out, reason);
}

int mjw_transcode_memory_progressive_at(const uint8_t *src, int len, unsigned flags, int o, int trim, const int *crop, int grey, const unsigned char *luma,
                                        const unsigned char *chroma, int coarsen_only, int progressive, unsigned char **out, size_t *out_len,
                                        int *rect_out, const char **reason)
{
	return transcode_memory_at(src, len, flags, o, trim, crop, grey, luma, chroma, coarsen_only, 0, 0, progressive, out, out_len, rect_out, NULL, reason);
}

int mjw_transcode_memory_window_at(const uint8_t *src, int len, unsigned flags, int o, int trim, const int *crop, int grey, const unsigned char *luma,
                                   const unsigned char *chroma, int coarsen_only, unsigned char **out, size_t *out_len, int *rect_out,
                                   const char **reason)
{
	return mjw_transcode_memory_restart_at(src, len, flags, o, trim, crop, grey, luma, chroma, coarsen_only, 0, 0, out, out_len, rect_out, NULL, reason);
}

int mjw_transcode_memory_requant_at(const uint8_t *src, int len, unsigned flags, int o, int trim, const unsigned char *luma,
                                    const unsigned char *chroma, int coarsen_only, unsigned char **out, size_t *out_len, const char **reason)
{
	return mjw_transcode_memory_window_at(src, len, flags, o, trim, NULL, 0, luma, chroma, coarsen_only, out, out_len, NULL, reason);
}

int mjw_transcode_memory_at(const uint8_t *src, int len, unsigned flags, int o, int trim, unsigned char **out, size_t *out_len, const char **reason)
{
	return mjw_transcode_memory_requant_at(src, len, flags, o, trim, NULL, NULL, 0, out, out_len, reason);
}

int mjh_transcode_memory(const uint8_t *src, int len, unsigned flags, unsigned char **out, size_t *out_len, const char **reason)
{
	return mjw_transcode_memory_at(src, len, flags, 1, 0, out, out_len, reason);
}
