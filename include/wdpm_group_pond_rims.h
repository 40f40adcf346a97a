/*
 * wdpm_group_pond_rims.h — the rim of every pond of a raster spread over the row blocks of a wdpm_group: the table of
 * wdpm_pond_rims.h, taken where the rows lie.  Product library only.  A fifth header, on the handle of wdpm_group_ponds.h.
 *
 * Definitions and table row are those of wdpm_pond_rims.h, unchanged.  The result equals, value for value and bit for bit, what
 * wdpm_rims_label and wdpm_rims_table give on a whole-raster context that holds the water wdpm_group_download_water returns.
 * Coordinates are padded coordinates of the WHOLE raster.  No water and no label comes to the host for it, and there is no
 * second context.
 *
 * Who counts which cell.  A pond cell gives its surface to its pond on the rank that owns its row.  A neighbour cell is handled
 * by the rank that owns its row and by that rank alone, for every pond it touches, whichever side of a row-block boundary those
 * ponds' cells lie on; the raster's two border rows belong to the first and to the last rank.  For this each rank is given the
 * whole-raster labels of the one row beyond either end of its owned rows (the host has them from the stitch) and nothing else
 * of its neighbours: a neighbour cell's level comes from its owner's DEM and water, never from a halo row.  A rank so holds
 * one rim row per pond it touches - its own, and the FOREIGN ponds it only borders on - and the host merges the ranks' rows:
 * extremes through the order-preserving image of a double, counts added, and of several rim cells at the lowest level the one
 * of the first rank, which is the one with the smallest padded index.
 *
 * Scope: the ranks of ONE process, as wdpm_group_ponds.h.  A group of one rank gives the single-context answer.
 */
#ifndef WDPM_GROUP_POND_RIMS_H
#define WDPM_GROUP_POND_RIMS_H

#include "wdpm_group_ponds.h"
#include "wdpm_pond_rims.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what the last wdpm_group_rims_label did */
typedef struct wdpm_group_rim_stats {
  int64_t ranks;          /* row blocks */
  int64_t slots;          /* sum over ranks of the rim rows a rank holds: its local ponds and its foreign ones */
  int64_t foreign;        /* sum over ranks of the ponds a rank holds a rim row for without owning a cell of them */
  double  merge_ms;       /* host time of the merge, milliseconds */
} wdpm_group_rim_stats;

/* wdpm_group_ponds_label, and the rim pass of every rank on the same water, from one call: every rank's labels, table, rim
 * kernels and transfers are queued before any rank is waited for.  Afterwards wdpm_group_ponds_table, _labels, _stats and
 * _rank_stats answer exactly as after wdpm_group_ponds_label.  Fails as that call fails, and when rim_cells or wall_cells of
 * a pond leave int64. */
int wdpm_group_rims_label(wdpm_group_ponds *h, double min_depth, int64_t *nponds);
/* the rim table of the last wdpm_group_rims_label: N rows; capacity < N fails and writes nothing.  Fails after a plain
 * wdpm_group_ponds_label, which leaves no rim table. */
int wdpm_group_rims_table(wdpm_group_ponds *h, wdpm_pond_rim *out, int64_t capacity);
int wdpm_group_rims_stats(wdpm_group_ponds *h, wdpm_group_rim_stats *out);
/* WDPM_RIMS_PHASES values for one rank, as wdpm_rims_phase_ms (the slot set-up counts with the rim pass); fails on a handle
 * made without WDPM_PONDS_TIMING=1.  The host's merge time is wdpm_group_rim_stats::merge_ms. */
int wdpm_group_rims_phase_ms(wdpm_group_ponds *h, int32_t rank, double *ms /* WDPM_RIMS_PHASES values */);

#ifdef __cplusplus
}
#endif
#endif
