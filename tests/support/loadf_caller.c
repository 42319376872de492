/*
 * loadf_caller.c -- a C program that uses the float loaders through include/image_api.h, the way a user of the reference
 * would: every stbi_loadf* entry point and every gamma / scale setter.  Compiled with -Wall -Werror by the tests, so the
 * prototypes of the header are checked against real calls (ctypes never reads them).
 *
 * usage: loadf_caller FILE.jpg   prints "ok W H COMP SUM" (SUM: the float sum of the default-gamma load) or "fail REASON"
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "image_api.h"

typedef struct {
	const unsigned char *p;
	int n, pos;
} mem_src;

static int cb_read(void *user, char *data, int size)
{
	mem_src *s = (mem_src *)user;
	int k = s->n - s->pos < size ? s->n - s->pos : size;
	memcpy(data, s->p + s->pos, (size_t)k);
	s->pos += k;
	return k;
}
static void cb_skip(void *user, int n) { ((mem_src *)user)->pos += n; }
static int cb_eof(void *user) { return ((mem_src *)user)->pos >= ((mem_src *)user)->n; }

int main(int argc, char **argv)
{
	stbi_io_callbacks cb = {cb_read, cb_skip, cb_eof};
	unsigned char *buf;
	long len;
	int x = 0, y = 0, comp = 0, x2, y2, c2, i, n;
	float *a, *b, *c, *d, *e;
	double sum = 0;
	FILE *f;
	mem_src src;
	if (argc < 2 || !(f = fopen(argv[1], "rb")))
		return 2;
	fseek(f, 0, SEEK_END);
	len = ftell(f);
	fseek(f, 0, SEEK_SET);
	buf = (unsigned char *)malloc((size_t)len);
	if (!buf || fread(buf, 1, (size_t)len, f) != (size_t)len)
		return 2;
	fclose(f);

	stbi_hdr_to_ldr_gamma(2.2f); /* link-compatibility setters: JPEG input never reads them */
	stbi_hdr_to_ldr_scale(1.0f);
	a = stbi_loadf_from_memory(buf, (int)len, &x, &y, &comp, 0);
	if (!a) {
		printf("fail %s\n", stbi_failure_reason());
		return 0;
	}
	n = x * y * comp;
	b = stbi_loadf(argv[1], &x2, &y2, &c2, 0);
	f = fopen(argv[1], "rb");
	c = f ? stbi_loadf_from_file(f, &x2, &y2, &c2, 0) : NULL;
	if (f)
		fclose(f);
	src.p = buf;
	src.n = (int)len;
	src.pos = 0;
	d = stbi_loadf_from_callbacks(&cb, &src, &x2, &y2, &c2, 0);
	if (!b || !c || !d || x2 != x || y2 != y || c2 != comp || memcmp(a, b, sizeof(float) * (size_t)n) || memcmp(a, c, sizeof(float) * (size_t)n) ||
		 memcmp(a, d, sizeof(float) * (size_t)n)) {
		printf("mismatch between the loaders\n");
		return 1;
	}
	/* gamma 1, scale 2: colour channels become 2 * v / 255 exactly as the reference computes it */
	stbi_ldr_to_hdr_gamma(1.0f);
	stbi_ldr_to_hdr_scale(2.0f);
	e = stbi_loadf_from_memory(buf, (int)len, &x2, &y2, &c2, 0);
	stbi_ldr_to_hdr_gamma(2.2f);
	stbi_ldr_to_hdr_scale(1.0f);
	if (!e || e[0] < a[0]) {
		printf("gamma / scale had no effect\n");
		return 1;
	}
	for (i = 0; i < n; ++i)
		sum += a[i];
	printf("ok %d %d %d %.6f\n", x, y, comp, sum);
	stbi_image_free(a);
	stbi_image_free(b);
	stbi_image_free(c);
	stbi_image_free(d);
	stbi_image_free(e);
	free(buf);
	return 0;
}
