/* mjh_exif_orientation under AddressSanitizer + UBSan (CPU build only): every record of a corpus file -- a 4-byte little-endian length,
 * then that many bytes -- is copied into a buffer of exactly its size and parsed.  Prints how many records gave each orientation.
 * Built and run by tests/test_exif_host.py. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mij_host.h"
int main(int argc, char **argv)
{
	long seen[9] = {0};
	FILE *f = argc > 1 ? fopen(argv[1], "rb") : NULL;
	if (!f)
		return 2;
	for (;;) {
		uint8_t h[4];
		if (fread(h, 1, 4, f) != 4)
			break;
		const uint32_t n = (uint32_t)h[0] | (uint32_t)h[1] << 8 | (uint32_t)h[2] << 16 | (uint32_t)h[3] << 24;
		uint8_t *buf = malloc(n ? n : 1);
		if (n && fread(buf, 1, n, f) != n) {
			free(buf);
			return 3;
		}
		const int o = mjh_exif_orientation(n ? buf : NULL, (int)n);
		free(buf);
		if (o < 1 || o > 8)
			return 4;
		seen[o]++;
	}
	fclose(f);
	for (int o = 1; o <= 8; ++o)
		printf("%d:%ld%s", o, seen[o], o < 8 ? " " : "\n");
	return 0;
}
