/* EXIF Orientation of a JPEG file (mjh_exif_orientation, mjh_exif_set_orientation, include/mij_host.h).  Reads nothing outside the
 * buffer and, inside the Exif APP1, nothing outside that segment: every offset is checked against the segment before it is followed.
 * Both calls make one walk (orientation_entry), so what one reads is what the other patches. */
#include <stdint.h>
#include <string.h>

#include "mij_host.h"

static uint32_t rd16(const uint8_t *p, int le) { return le ? (uint32_t)p[0] | (uint32_t)p[1] << 8 : (uint32_t)p[0] << 8 | (uint32_t)p[1]; }

static uint32_t rd32(const uint8_t *p, int le)
{
	return le ? (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24
				 : (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3];
}

/* the two value bytes of the Orientation entry of IFD0 of the TIFF block t[0, n), and the block's byte order; NULL when there is no
 * such entry of one SHORT */
static const uint8_t *tiff_orientation(const uint8_t *t, uint32_t n, int *le_out)
{
	int le;
	if (n < 8)
		return NULL;
	if (t[0] == 'I' && t[1] == 'I' && t[2] == 42 && t[3] == 0)
		le = 1;
	else if (t[0] == 'M' && t[1] == 'M' && t[2] == 0 && t[3] == 42)
		le = 0;
	else
		return NULL;
	const uint32_t ifd = rd32(t + 4, le);
	if (ifd < 8 || ifd > n || n - ifd < 2)
		return NULL;
	const uint32_t cnt = rd16(t + ifd, le);
	if ((uint64_t)cnt * 12u > (uint64_t)(n - ifd - 2))
		return NULL; /* the directory runs past the segment */
	for (uint32_t i = 0; i < cnt; ++i) {
		const uint8_t *e = t + ifd + 2 + 12u * i;
		if (rd16(e, le) != 0x0112)
			continue;
		if (rd16(e + 2, le) != 3 || rd32(e + 4, le) != 1)
			return NULL; /* not one SHORT */
		*le_out = le;
		return e + 8;
	}
	return NULL;
}

/* the walk over the marker segments to the first Exif APP1 */
static const uint8_t *orientation_entry(const uint8_t *buf, int len, int *le)
{
	if (!buf || len < 4 || buf[0] != 0xFF || buf[1] != 0xD8)
		return NULL;
	const size_t n = (size_t)len;
	size_t i = 2;
	for (;;) {
		if (i >= n || buf[i] != 0xFF)
			return NULL;
		while (i < n && buf[i] == 0xFF) /* fill bytes */
			++i;
		if (i >= n)
			return NULL;
		const uint8_t m = buf[i++];
		if (m == 0xDA || m == 0xD9 || m == 0x00)
			return NULL; /* SOS, EOI: no more header segments; FF00 is no marker */
		if (m == 0x01 || m == 0xD8 || (m >= 0xD0 && m <= 0xD7))
			continue; /* markers without a length */
		if (n - i < 2)
			return NULL;
		const size_t sl = (size_t)buf[i] << 8 | buf[i + 1];
		if (sl < 2 || sl > n - i)
			return NULL;
		if (m == 0xE1 && sl >= 2 + 6 && memcmp(buf + i + 2, "Exif\0\0", 6) == 0)
			return tiff_orientation(buf + i + 8, (uint32_t)(sl - 8), le);
		i += sl;
	}
}

int mjh_exif_orientation(const uint8_t *buf, int len)
{
	int le = 0;
	const uint8_t *e = orientation_entry(buf, len, &le);
	if (!e)
		return 1;
	const uint32_t v = rd16(e, le);
	return v >= 1 && v <= 8 ? (int)v : 1;
}

int mjh_exif_set_orientation(uint8_t *buf, int len, int value)
{
	int le = 0;
	if (value < 1 || value > 8)
		return 0;
	const uint8_t *e = orientation_entry(buf, len, &le);
	if (!e)
		return 0;
	uint8_t *w = buf + (e - buf);
	w[le ? 0 : 1] = (uint8_t)value;
	w[le ? 1 : 0] = 0;
	return 1;
}
