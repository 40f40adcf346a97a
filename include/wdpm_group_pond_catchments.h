/*
 * wdpm_group_pond_catchments.h — the catchment of every pond of a raster spread over the row blocks of a wdpm_group: basin raster
 * and table of wdpm_pond_catchments.h, taken where the rows lie.  Product library only.  A seventh header, on the handle of
 * wdpm_group_ponds.h.
 *
 * Definitions and table row are those of wdpm_pond_catchments.h, unchanged: level, slope cell, receiver, tie rule, pit, basin.
 * The result equals, value for value (head_level bit for bit), what wdpm_catch_label, wdpm_catch_table, wdpm_catch_basins and
 * wdpm_catch_stats give on a whole-raster context that holds the water wdpm_group_download_water returns.  Coordinates are padded
 * coordinates of the WHOLE raster.  No water, label or link raster comes to the host for it, and there is no second context.
 *
 * Who computes what.  A rank takes the receiver of every cell of its owned rows and of those alone.  Of the one row beyond either
 * end it is given the whole-raster labels (as the rim pass is) and the 64-bit level keys its owner wrote from its own DEM and
 * water: a halo row's DEM and water are never read.  A slope cell whose receiver is a pond cell of such a row drains into that
 * pond and is counted as its inflow cell by the rank that owns the slope cell.  Where the receiver is a slope cell of such a
 * row, the descent EXITS the rank; after the ranks' jump rounds the host follows the exits from seam row to seam row (two rows of
 * links per rank come down) and hands every rank the end of each of its exits.  Through exits a rank's cells can drain to a pond
 * the rank neither owns nor borders on - a REMOTE pond, for which it then holds a table row as well.  The host adds the ranks'
 * rows up.
 *
 * Scope: the ranks of ONE process, as wdpm_group_ponds.h.  A group of one rank gives the single-context answer.
 */
#ifndef WDPM_GROUP_POND_CATCHMENTS_H
#define WDPM_GROUP_POND_CATCHMENTS_H

#include "wdpm_group_pond_rims.h"
#include "wdpm_pond_catchments.h"

#ifdef __cplusplus
extern "C" {
#endif

/* of the last wdpm_group_catch_label: the five counts of wdpm_pond_catchment_stats for the whole raster, then the group's own */
typedef struct wdpm_group_catchment_stats {
  int64_t slope_cells;
  int64_t pit_cells;
  int64_t unponded_cells;
  int64_t rounds;            /* launches of the jump kernel on the rank that took the most */
  int64_t ponds;
  int64_t ranks;             /* row blocks */
  int64_t exits;             /* owned cells whose descent left their rank's rows, summed over ranks */
  int64_t crossings;         /* cells of the ranks' first and last owned rows that held an exit: the nodes the host followed */
  int64_t remote;            /* sum over ranks of the ponds a rank's cells drain to without the rank owning or bordering them */
  double  resolve_ms;        /* host time of following the exits and of the merge, milliseconds */
} wdpm_group_catchment_stats;

/* wdpm_group_rims_label, and the catchment pass of every rank on the same water, from one call.  Afterwards wdpm_group_ponds_*
 * and wdpm_group_rims_table answer exactly as after wdpm_group_rims_label.  A later wdpm_group_ponds_label or
 * wdpm_group_rims_label takes the catchment table away.  Fails as those calls fail, when the whole raster holds so many ponds that
 * pond codes and exit codes of a link would meet (N + 2 * (ncols + 2) + 2 > 2^31), when a rank needs more than 40 jump rounds, and
 * when a count leaves int64. */
int wdpm_group_catch_label(wdpm_group_ponds *h, double min_depth, int64_t *nponds);
/* the catchment table of the last wdpm_group_catch_label: N rows; capacity < N fails and writes nothing */
int wdpm_group_catch_table(wdpm_group_ponds *h, wdpm_pond_catchment *out, int64_t capacity);
/* basin(c) of the last wdpm_group_catch_label: (nrows + 2) x (ncols + 2) int32, every rank's owned rows where they lie in the
 * whole raster, as wdpm_group_ponds_labels lays them out */
int wdpm_group_catch_basins(wdpm_group_ponds *h, int32_t *padded);
int wdpm_group_catch_stats(wdpm_group_ponds *h, wdpm_group_catchment_stats *out);
/* WDPM_CATCH_PHASES values for one rank, as wdpm_catch_phase_ms (the table's initialisation counts with the receivers, the slots of
 * remote ponds with the tally; the seam keys, 2 x (ncols + 2) cells, are not timed); fails on a handle made without
 * WDPM_PONDS_TIMING=1.  The host's time is wdpm_group_catchment_stats::resolve_ms. */
int wdpm_group_catch_phase_ms(wdpm_group_ponds *h, int32_t rank, double *ms /* WDPM_CATCH_PHASES values */);

#ifdef __cplusplus
}
#endif
#endif
