/*
 * wdpm_group_pond_outlets.h — the outlet of every pond of a raster spread over the row blocks of a wdpm_group: the table of
 * wdpm_pond_outlets.h, taken where the rows lie.  Product library only.  An eighth header, on the handle of wdpm_group_ponds.h.
 *
 * Definitions and table row are those of wdpm_pond_outlets.h, unchanged: pass, outlet, tie rule, pour_level, divide_cells,
 * fill_cells, fill_q.  The result equals, value for value (pour_level bit for bit), what wdpm_outlets_table and wdpm_outlets_stats
 * give on a whole-raster context that holds the water wdpm_group_download_water returns.  Coordinates are padded coordinates of
 * the WHOLE raster.  No water, label or basin raster comes to the host for it, and there is no second context.
 *
 * Who computes what.  A rank takes every pass (a, b) whose a lies in its owned rows; b may lie in the one row beyond either end,
 * of which the rank is given the whole-raster basins (each rank's first and last owned row of basins go to the rank that faces
 * them) and the level keys its owner wrote for the catchment pass: a halo row's DEM and water are never read.  The pour level of a
 * pond is final only over all ranks, so the host stands between the two device passes: the ranks' lowest passes come down, the
 * lowest per pond goes back up, and then every rank fills its own cells to that level and offers its first pair at that height.
 * The lowest rank that offered holds the smallest whole-raster index, which is the tie rule.  The host adds the ranks' rows up.
 *
 * Scope: the ranks of ONE process, as wdpm_group_ponds.h.  A group of one rank gives the single-context answer.
 */
#ifndef WDPM_GROUP_POND_OUTLETS_H
#define WDPM_GROUP_POND_OUTLETS_H

#include "wdpm_group_pond_catchments.h"
#include "wdpm_pond_outlets.h"

#ifdef __cplusplus
extern "C" {
#endif

/* of the last wdpm_group_outlets_label: the four counts of wdpm_pond_outlet_stats for the whole raster, then the group's own */
typedef struct wdpm_group_outlet_stats {
  int64_t ponds;
  int64_t no_outlet;
  int64_t to_land;
  int64_t divide_cells;
  int64_t ranks;             /* row blocks */
  int64_t seam_outlets;      /* ponds whose outlet pair (a, b) lies in two ranks' rows */
  int64_t split_ponds;       /* ponds for which more than one rank held divide or fill cells */
  double  merge_ms;          /* host time of both merges, milliseconds */
} wdpm_group_outlet_stats;

/* wdpm_group_catch_label, and the outlet pass of every rank on the same water, from one call.  Afterwards every older
 * wdpm_group_* query answers exactly as after wdpm_group_catch_label; wdpm_group_catch_basins still returns owned rows only.  A
 * later wdpm_group_ponds_label, wdpm_group_rims_label or wdpm_group_catch_label takes the outlet table away.  A call that fails -
 * as those calls fail, over a fill term of 512 m or more or one that is not finite on any rank, over memory, over a device error,
 * over a sum that leaves 64 bits - leaves the handle without any table; the handle itself stays usable. */
int wdpm_group_outlets_label(wdpm_group_ponds *h, double min_depth, int64_t *nponds);
/* the outlet table of the last wdpm_group_outlets_label: N rows; capacity < N fails and writes nothing */
int wdpm_group_outlets_table(wdpm_group_ponds *h, wdpm_pond_outlet *out, int64_t capacity);
int wdpm_group_outlets_stats(wdpm_group_ponds *h, wdpm_group_outlet_stats *out);
/* WDPM_OUTLETS_PHASES values for one rank, as wdpm_outlets_phase_ms (the seam basins on their way up count with the passes, the
 * pour keys on their way up with the locate pass); fails on a handle made without WDPM_PONDS_TIMING=1.  The host's time is
 * wdpm_group_outlet_stats::merge_ms. */
int wdpm_group_outlets_phase_ms(wdpm_group_ponds *h, int32_t rank, double *ms /* WDPM_OUTLETS_PHASES values */);

#ifdef __cplusplus
}
#endif
#endif
