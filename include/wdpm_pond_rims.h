/*
 * wdpm_pond_rims.h — the rim of every pond of the inventory (include/wdpm_ponds.h): spill level, shoreline, walls and the
 * spread of the water surface, one table row per pond.  Product library only, conventions as in wdpm_ponds.h.
 *
 * Definitions (exact: every result is an integer or an exact double, bit-reproducible whatever order the device visits the
 * cells in).  L is the label raster of the call, dem the device DEM (NODATA and border are +inf), w the water that was labelled.
 *   surface      of a pond cell: dem + w (one fp64 addition); surface_min / surface_max are its extremes over the pond
 *   neighbour    of pond k: a cell with L == 0 that has at least one of its eight neighbours in pond k.  Border and NODATA cells
 *                are cells here.  A neighbour counts once per pond, and for every pond it touches (at most four)
 *   rim cell     a neighbour with dem < +inf; its level is (w > 0) ? dem + w : dem (NaN, negative and zero water fall to dem;
 *                water at or below min_depth counts).  rim_cells is their number: the length of the shoreline
 *   rim_level    the minimum level over the pond's rim cells, compared through the order-preserving 64-bit image of a double
 *                (-0.0 sorts below +0.0): the spill point.  rim_row, rim_col: the rim cell that holds it, padded coordinates;
 *                of several the one with the smallest padded row-major index.  No rim cell: +inf, -1, -1
 *   wall cell    a neighbour with !(dem < +inf): border, NODATA or a NaN elevation.  wall_cells is their number
 *   freeboard    rim_level - surface_max, for the caller to take: +inf without a rim, <= 0 on a pond that is still spilling
 */
#ifndef WDPM_POND_RIMS_H
#define WDPM_POND_RIMS_H

#include "wdpm_ponds.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one table row: pond k is row k - 1; 48 bytes */
typedef struct wdpm_pond_rim {
  double  surface_min, surface_max;
  double  rim_level;
  int32_t rim_row, rim_col;
  int64_t rim_cells, wall_cells;
} wdpm_pond_rim;

/* wdpm_ponds_label, then the rim pass on the same water, queued on the context's stream with nothing in between: label raster
 * and water belong together.  Afterwards wdpm_ponds_table, wdpm_ponds_labels and wdpm_ponds_stats answer as after
 * wdpm_ponds_label.  Handles of wdpm_ponds_create; a raster spread over row blocks has wdpm_group_rims_label
 * (wdpm_group_pond_rims.h). */
int wdpm_rims_label(wdpm_ponds *h, double min_depth, int64_t *nponds);
/* the rim table of the last wdpm_rims_label: N rows; capacity < N fails and writes nothing.  Fails after a plain
 * wdpm_ponds_label, which leaves no rim table. */
int wdpm_rims_table(wdpm_ponds *h, wdpm_pond_rim *out, int64_t capacity);
/* With WDPM_PONDS_TIMING=1 set when the handle was made: milliseconds of the rim pass (with its initialisation) and of the
 * locate pass (with the finish) of the last wdpm_rims_label. */
#define WDPM_RIMS_PHASES 2
int wdpm_rims_phase_ms(wdpm_ponds *h, double *ms /* WDPM_RIMS_PHASES values */);

#ifdef __cplusplus
}
#endif
#endif
