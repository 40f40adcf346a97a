/* wdpmcl_ponds.h - the pond files of the WDPMCL command line (wdpmcl_ponds.c): what wdpmcl_main.c knows of ponds. */
#ifndef WDPMCL_PONDS_H
#define WDPMCL_PONDS_H
#include "../../include/wdpm.h"

/* the pond files asked for in the environment, taken on the group before it goes (on its one context, or over its `ndev` row
 * blocks); returns non-zero when a file that was asked for was not written; *guard_bad as wdpm_*_ponds_guard_bad says under
 * WDPM_GUARD_KB, else 0.  `phase` (WDPM_TIMING) is called before and after the inventory, and only when one is taken. */
int wdpmcl_pond_files(wdpm_group *grp, int ndev, double cellarea, int64_t *guard_bad, void (*phase)(const char *name));

#endif
