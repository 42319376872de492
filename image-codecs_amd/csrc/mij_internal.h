/*
 * mij_internal.h -- what the library's own host stages share with the runtime and no caller may use: not installed, not in include/.
 */
#ifndef MIJ_INTERNAL_H
#define MIJ_INTERNAL_H

#include <stddef.h>
#include <stdint.h>
#include "mij.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Hands a slot the row-extent table (mij.h, "row-extent table") of the staging its producer has just written: n = the sum of comp[c].bh
 * bytes, component after component, entries above 3 read as 3.  INTERNAL: the band kernels skip the coefficient chunks an entry rules
 * out, so a table that claims less than the planes hold changes pixels.  Only a producer that wrote every block of the slot's rows
 * itself calls it, behind its last write -- the host walk of batch_decode.c, and the Python binding's twin of it (Batch.add_jpeg) --
 * and mij_batch_stage_region / mij_batch_coef take the table back to 3.  Clones cannot be given one (MIJ_E_ARG).
 */
int mij_batch_set_row_classes(mij_batch *b, int slot, const uint8_t *classes, size_t n);

#ifdef __cplusplus
}
#endif

#endif
