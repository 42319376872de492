/*
 * transcode_orient.c -- mjh_transcode_memory_oriented, mjh_transcode_memory_requant and mjh_transcode_memory_window (include/mij_host.h):
 * the transcode on the host with an orientation applied, the file's own EXIF tag included, and optionally a crop, greyscale and new
 * quantisation tables.  The transforms themselves are transcode_host.c's (mjw_tplan_oriented, mjw_units_orient, mjw_tplan_cropped,
 * mjw_transcode_memory_window_at); this file adds what needs the EXIF walk (exif.c), so that transcode_host.c links without it.
 */
#include <limits.h>

#include "mij_host.h"

static int transcode_memory(const uint8_t *src, int len, unsigned flags, int o, int trim, const int *crop, int grey, const unsigned char *luma,
                            const unsigned char *chroma, int coarsen_only, int restart_rows, int restart_mcus, int progressive, unsigned char **out,
                            size_t *out_len, int *rect_out, int *ri_out, const char **reason)
{
	if (o < 0 || o > 8) {
		if (out)
			*out = NULL;
		if (out_len)
			*out_len = 0;
		if (reason)
			*reason = "orientation is not 0 (the file's tag) or 1..8";
		return 0;
	}
	if (o == 0)
		o = mjh_exif_orientation(src, len);
	if (!(progressive ? mjw_transcode_memory_progressive_at(src, len, flags, o, trim, crop, grey, luma, chroma, coarsen_only, progressive, out, out_len,
																			  rect_out, reason)
							: mjw_transcode_memory_restart_at(src, len, flags, o, trim, crop, grey, luma, chroma, coarsen_only, restart_rows, restart_mcus, out,
																		 out_len, rect_out, ri_out, reason)))
		return 0;
	/* the picture is upright now: a copied tag that still said otherwise would turn it a second time */
	if ((flags & MJW_COPY_MARKERS) && o != 1)
		(void)mjh_exif_set_orientation(*out, *out_len > (size_t)INT_MAX ? INT_MAX : (int)*out_len, 1);
	return 1;
}

int mjh_transcode_memory_restart_by(const uint8_t *src, int len, unsigned flags, int o, int trim, const int *crop, int grey, const unsigned char *luma,
                                    const unsigned char *chroma, int coarsen_only, int restart_rows, int restart_mcus, unsigned char **out,
                                    size_t *out_len, int *rect_out, int *ri_out, const char **reason)
{
	return transcode_memory(src, len, flags, o, trim, crop, grey, luma, chroma, coarsen_only, restart_rows, restart_mcus, 0, out, out_len, rect_out, ri_out,
									reason);
}

int mjh_transcode_memory_progressive(const uint8_t *src, int len, unsigned flags, int o, int trim, const int *crop, int grey, const unsigned char *luma,
                                     const unsigned char *chroma, int coarsen_only, int progressive, unsigned char **out, size_t *out_len,
                                     int *rect_out, const char **reason)
{
	return transcode_memory(src, len, flags, o, trim, crop, grey, luma, chroma, coarsen_only, 0, 0, progressive, out, out_len, rect_out, NULL, reason);
}

int mjh_transcode_memory_restart(const uint8_t *src, int len, unsigned flags, int o, int trim, const int *crop, int grey, const unsigned char *luma,
                                 const unsigned char *chroma, int coarsen_only, unsigned char **out, size_t *out_len, int *rect_out, int ri,
                                 const char **reason)
{
	return mjh_transcode_memory_restart_by(src, len, flags, o, trim, crop, grey, luma, chroma, coarsen_only, 0, ri, out, out_len, rect_out, NULL, reason);
}

int mjh_transcode_memory_window(const uint8_t *src, int len, unsigned flags, int o, int trim, const int *crop, int grey, const unsigned char *luma,
                                const unsigned char *chroma, int coarsen_only, unsigned char **out, size_t *out_len, int *rect_out,
                                const char **reason)
{
	return mjh_transcode_memory_restart_by(src, len, flags, o, trim, crop, grey, luma, chroma, coarsen_only, 0, 0, out, out_len, rect_out, NULL, reason);
}

int mjh_transcode_memory_requant(const uint8_t *src, int len, unsigned flags, int o, int trim, const unsigned char *luma,
                                 const unsigned char *chroma, int coarsen_only, unsigned char **out, size_t *out_len, const char **reason)
{
	return mjh_transcode_memory_window(src, len, flags, o, trim, NULL, 0, luma, chroma, coarsen_only, out, out_len, NULL, reason);
}

int mjh_transcode_memory_oriented(const uint8_t *src, int len, unsigned flags, int o, int trim, unsigned char **out, size_t *out_len,
                                  const char **reason)
{
	return mjh_transcode_memory_requant(src, len, flags, o, trim, NULL, NULL, 0, out, out_len, reason);
}
