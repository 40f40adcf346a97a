/*
 * wdpm_group_ponds.h — pond inventory of a raster spread over the row blocks of a wdpm_group (product library only).
 *
 * A third header beside wdpm.h and wdpm_ponds.h: conventions, definitions and table row are those of wdpm_ponds.h.  The handle
 * labels the water wdpm_group_download_water would return - every rank's owned rows with the owed threshold flush and the owed
 * drain() applied - exactly as a wdpm_ponds handle labels a whole-raster context that holds the same water: the same ponds, the
 * same numbering 1..N by first cell, the same table, value for value.  Coordinates are padded coordinates of the WHOLE raster,
 * labels int32 in its padded layout (nrows + 2) x (ncols + 2).
 *
 * Every rank labels its owned rows where they lie, with the kernels of the single-context inventory and all ranks queued before
 * any is waited for; the labels of the rows either side of each row-block boundary come to the host with the ranks' pond counts,
 * the host joins what touches there and numbers the whole, and each rank's table kernel then stores whole-raster labels: one
 * store per cell, no relabelling pass.  The ranks' tables are merged on the host.
 *
 * Scope: the ranks of ONE process (wdpm_group_*).  Ranks living in separate processes (wdpm_rank_* over a host transport or
 * RCCL) have no inventory here.  A group of one rank gives the single-context answer through the same calls.
 */
#ifndef WDPM_GROUP_PONDS_H
#define WDPM_GROUP_PONDS_H

#include "wdpm_ponds.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wdpm_group_ponds wdpm_group_ponds; /* opaque */

/* what the last wdpm_group_ponds_label did */
typedef struct wdpm_group_pond_stats {
  int64_t ranks;          /* row blocks */
  int64_t ponds;          /* N of the whole raster */
  int64_t local_ponds;    /* sum of the ranks' own counts */
  int64_t stitch_unions;  /* pairs of touching runs across a row-block boundary (whole-row runs, 8-connectivity), each joined */
  int64_t merged;         /* local ponds that gave up their number to a pond beginning higher up: ponds == local_ponds - merged */
  double  stitch_ms;      /* host time of the join and the numbering, milliseconds */
} wdpm_group_pond_stats;

/* WDPM_GUARD_KB, WDPM_PONDS_ROWS_PER_WAVE and WDPM_PONDS_TIMING are read when the handle is made, as wdpm_ponds_create reads
 * them.  A rank whose owned rows with one row either side hold more than 2^31 - 1 cells is refused.  Destroy the handle before
 * its group. */
int  wdpm_group_ponds_create(wdpm_group_ponds **out, wdpm_group *grp);
void wdpm_group_ponds_destroy(wdpm_group_ponds *h);
/* label, number and accumulate over all ranks; min_depth finite and >= 0 (metres).  Fails (and leaves the handle without an
 * inventory) on a pond cell of >= 512 m, on 2^31 ponds or more, and when cells or volume_q of a joined pond overflow. */
int  wdpm_group_ponds_label(wdpm_group_ponds *h, double min_depth, int64_t *nponds);
/* the table of the last label call: N rows; capacity < N fails and writes nothing */
int  wdpm_group_ponds_table(wdpm_group_ponds *h, wdpm_pond *out, int64_t capacity);
/* the label raster of the last label call: (nrows + 2) x (ncols + 2) int32, every rank's owned rows */
int  wdpm_group_ponds_labels(wdpm_group_ponds *h, int32_t *padded);
/* guard bytes around all ranks' inventory buffers that no longer hold their fill (0 without WDPM_GUARD_KB) */
int  wdpm_group_ponds_guard_bad(wdpm_group_ponds *h, int64_t *bytes);
int  wdpm_group_ponds_stats(wdpm_group_ponds *h, wdpm_group_pond_stats *out);
/* one rank's own labelling: segments, unions and ponds of its rows alone */
int  wdpm_group_ponds_rank_stats(wdpm_group_ponds *h, int32_t rank, wdpm_pond_stats *out);
/* WDPM_PONDS_PHASES values for one rank, as wdpm_ponds_phase_ms (the seam-label kernel counts as scan); fails on a handle made
 * without WDPM_PONDS_TIMING=1.  The host's stitch time is wdpm_group_pond_stats::stitch_ms. */
int  wdpm_group_ponds_phase_ms(wdpm_group_ponds *h, int32_t rank, double *ms);

#ifdef __cplusplus
}
#endif
#endif
