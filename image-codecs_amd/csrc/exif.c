/* EXIF Orientation of a JPEG file (mjh_exif_orientation, include/mij_host.h).  Reads nothing outside the buffer and, inside the Exif
 * APP1, nothing outside that segment: every offset is checked against the segment before it is followed. */
#include <stdint.h>
#include <string.h>

#include "mij_host.h"

static uint32_t rd16(const uint8_t *p, int le) { return le ? (uint32_t)p[0] | (uint32_t)p[1] << 8 : (uint32_t)p[0] << 8 | (uint32_t)p[1]; }

static uint32_t rd32(const uint8_t *p, int le)
{
	return le ? (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24
				 : (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3];
}

/* the Orientation of IFD0 of the TIFF block t[0, n) */
static int tiff_orientation(const uint8_t *t, uint32_t n)
{
	int le;
	if (n < 8)
		return 1;
	if (t[0] == 'I' && t[1] == 'I' && t[2] == 42 && t[3] == 0)
		le = 1;
	else if (t[0] == 'M' && t[1] == 'M' && t[2] == 0 && t[3] == 42)
		le = 0;
	else
		return 1;
	const uint32_t ifd = rd32(t + 4, le);
	if (ifd < 8 || ifd > n || n - ifd < 2)
		return 1;
	const uint32_t cnt = rd16(t + ifd, le);
	if ((uint64_t)cnt * 12u > (uint64_t)(n - ifd - 2))
		return 1; /* the directory runs past the segment */
	for (uint32_t i = 0; i < cnt; ++i) {
		const uint8_t *e = t + ifd + 2 + 12u * i;
		if (rd16(e, le) != 0x0112)
			continue;
		if (rd16(e + 2, le) != 3 || rd32(e + 4, le) != 1)
			return 1; /* not one SHORT */
		const uint32_t v = rd16(e + 8, le);
		return v >= 1 && v <= 8 ? (int)v : 1;
	}
	return 1;
}

int mjh_exif_orientation(const uint8_t *buf, int len)
{
	if (!buf || len < 4 || buf[0] != 0xFF || buf[1] != 0xD8)
		return 1;
	const size_t n = (size_t)len;
	size_t i = 2;
	for (;;) {
		if (i >= n || buf[i] != 0xFF)
			return 1;
		while (i < n && buf[i] == 0xFF) /* fill bytes */
			++i;
		if (i >= n)
			return 1;
		const uint8_t m = buf[i++];
		if (m == 0xDA || m == 0xD9 || m == 0x00)
			return 1; /* SOS, EOI: no more header segments; FF00 is no marker */
		if (m == 0x01 || m == 0xD8 || (m >= 0xD0 && m <= 0xD7))
			continue; /* markers without a length */
		if (n - i < 2)
			return 1;
		const size_t sl = (size_t)buf[i] << 8 | buf[i + 1];
		if (sl < 2 || sl > n - i)
			return 1;
		if (m == 0xE1 && sl >= 2 + 6 && memcmp(buf + i + 2, "Exif\0\0", 6) == 0)
			return tiff_orientation(buf + i + 8, (uint32_t)(sl - 8));
		i += sl;
	}
}
