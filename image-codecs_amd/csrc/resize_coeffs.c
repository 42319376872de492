/* Coefficients of the resized tensor output (mij_batch_set_out_tensor_resized, include/mij.h): one axis, in doubles, then fixed point
 * with 22 fraction bits.  Compiled with -ffp-contract=off and evaluated with libm's sin / cos, so that tests/resize_model.py -- the
 * same expressions in Python doubles -- reproduces every integer. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "mij.h"
#include "mij_host.h"

static double sinc(double x)
{
	if (x == 0.0)
		return 1.0;
	x = x * M_PI;
	return sin(x) / x;
}

static double filter(int f, double x)
{
	switch (f) {
	case MIJ_FILTER_BOX:
		return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;
	case MIJ_FILTER_BILINEAR:
		if (x < 0.0)
			x = -x;
		return x < 1.0 ? 1.0 - x : 0.0;
	case MIJ_FILTER_HAMMING:
		if (x < 0.0)
			x = -x;
		if (x == 0.0)
			return 1.0;
		if (x >= 1.0)
			return 0.0;
		x = x * M_PI;
		return sin(x) / x * (0.54f + 0.46f * cos(x));
	case MIJ_FILTER_BICUBIC: {
		const double a = -0.5;
		if (x < 0.0)
			x = -x;
		if (x < 1.0)
			return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
		if (x < 2.0)
			return (((x - 5) * x + 8) * x - 4) * a;
		return 0.0;
	}
	default: /* MIJ_FILTER_LANCZOS */
		return (-3.0 <= x && x < 3.0) ? sinc(x) * sinc(x / 3) : 0.0;
	}
}

static const double k_support[5] = {0.5, 1.0, 1.0, 2.0, 3.0};

int mjh_resize_coeffs(int in, int out, int filt, int32_t *lo_n, int32_t *k, size_t cap)
{
	if (in < 1 || in > (1 << 24) || out < 1 || out > (1 << 24) || filt < MIJ_FILTER_BOX || filt > MIJ_FILTER_LANCZOS)
		return MIJ_E_ARG;
	const double scale = (double)in / out, fs = scale < 1.0 ? 1.0 : scale, support = k_support[filt] * fs;
	const int ksize = (int)ceil(support) * 2 + 1;
	if (!lo_n || !k || cap < (size_t)out * (size_t)ksize)
		return ksize;
	for (int o = 0; o < out; ++o) {
		const double center = (o + 0.5) * scale;
		int lo = (int)(center - support + 0.5), hi = (int)(center + support + 0.5);
		if (lo < 0)
			lo = 0;
		if (hi > in)
			hi = in;
		const int n = hi - lo;
		int32_t *kk = k + (size_t)o * ksize;
		double ww = 0.0; /* summed in order t = 0..n-1; each weight is evaluated again below (the same value) */
		for (int t = 0; t < n; ++t)
			ww += filter(filt, (t + lo - center + 0.5) / fs);
		for (int t = 0; t < n; ++t) {
			double v = filter(filt, (t + lo - center + 0.5) / fs);
			if (ww != 0.0)
				v /= ww;
			kk[t] = (int32_t)(v * (1 << 22) + (v < 0 ? -0.5 : 0.5));
		}
		for (int t = n; t < ksize; ++t)
			kk[t] = 0;
		lo_n[2 * o] = lo;
		lo_n[2 * o + 1] = n;
	}
	return ksize;
}
