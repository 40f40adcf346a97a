/*
 * wdpm_pond_catchments.h — the catchment of every pond of the inventory (include/wdpm_ponds.h): which pond every dry cell drains
 * to, one int32 per cell, and one table row per pond.  Product library only, conventions as in wdpm_ponds.h and wdpm_pond_rims.h.
 *
 * Definitions (exact: every result is an integer or an exact double, bit-reproducible whatever order the device visits the
 * cells in).  L is the label raster of the call, dem the device DEM (NODATA and border are +inf), w the water that was labelled.
 * Doubles are compared through the order-preserving 64-bit image of a double that max_depth and rim_level use (-0.0 below +0.0).
 *   level        of a cell with dem < +inf (no other cell has one): dem + w (one fp64 addition) on a pond cell, and
 *                (w > 0) ? dem + w : dem on any other - the rim cell's rule: water at or below min_depth counts; NaN, zero and
 *                negative water fall to dem
 *   slope cell   L == 0 and dem < +inf.  Interior by construction
 *   receiver     of a slope cell: the neighbour of lowest level among the eight neighbours that have a level, provided that level
 *                is STRICTLY below the cell's own; among equals the one of smallest padded row-major index (up-left, up, up-right,
 *                left, right, down-left, down, down-right).  No distance weighting: the drop to a diagonal neighbour counts like
 *                the drop to a straight one.  That keeps every result exact, and it is the model's own notion of downhill: the
 *                stencil of the iteration moves water to all eight neighbours alike
 *   pit          a slope cell without a receiver.  Flats are NOT resolved: every cell of a flat that has no lower neighbour is
 *                a pit of its own
 *   descent      from a slope cell, follow receivers.  Levels fall strictly, so the path is finite and has no cycle; it ends at
 *                the first pond cell it meets or at a pit
 *   basin(c)     k > 0: c is a cell of pond k, or a slope cell whose descent ends in pond k;  0: a pit, or a slope cell whose
 *                descent ends in a pit;  -1: a cell without a level (border, NODATA, NaN elevation)
 *   catch_cells  of pond k: the slope cells with basin == k (pond cells are not counted)
 *   inflow_cells the slope cells whose RECEIVER is a cell of pond k: where the land's water enters
 *   head_level   the highest level over the pond's catch_cells; -inf when there is none
 *   row_min ...  the bounding box of the pond's cells and its catchment together, padded coordinates
 * For every call:  sum of wdpm_pond.cells + sum of catch_cells + unponded_cells == number of cells with dem < +inf.
 */
#ifndef WDPM_POND_CATCHMENTS_H
#define WDPM_POND_CATCHMENTS_H

#include "wdpm_pond_rims.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one table row: pond k is row k - 1; 40 bytes */
typedef struct wdpm_pond_catchment {
  int64_t catch_cells, inflow_cells;
  double  head_level;
  int32_t row_min, row_max, col_min, col_max;
} wdpm_pond_catchment;

/* of the last wdpm_catch_label */
typedef struct wdpm_pond_catchment_stats {
  int64_t slope_cells;       /* L == 0 and dem < +inf */
  int64_t pit_cells;         /* slope cells without a receiver */
  int64_t unponded_cells;    /* slope cells with basin == 0, pits included */
  int64_t rounds;            /* launches of the jump kernel */
  int64_t ponds;
} wdpm_pond_catchment_stats;

/* wdpm_rims_label, then the catchment pass on the same water, queued on the context's stream with nothing in between: labels,
 * pond table, rim table, catchment table and basin raster belong to the same water, and wdpm_ponds_*, wdpm_rims_table answer as
 * after wdpm_rims_label.  A later wdpm_ponds_label or wdpm_rims_label takes the catchment table away.  Handles of
 * wdpm_ponds_create only: descents cross row blocks.  The descents are shortened by pointer jumping in rounds; a call that would
 * need more than 40 rounds (no raster of fewer than 2^31 cells does) fails with a message. */
int wdpm_catch_label(wdpm_ponds *h, double min_depth, int64_t *nponds);
/* the catchment table of the last wdpm_catch_label: N rows; capacity < N fails and writes nothing */
int wdpm_catch_table(wdpm_ponds *h, wdpm_pond_catchment *out, int64_t capacity);
/* basin(c) of the last wdpm_catch_label: rows x (ncols + 2) int32, the padded layout of wdpm_ponds_labels */
int wdpm_catch_basins(wdpm_ponds *h, int32_t *padded);
int wdpm_catch_stats(wdpm_ponds *h, wdpm_pond_catchment_stats *out);
/* With WDPM_PONDS_TIMING=1 set when the handle was made: milliseconds of the receiver pass, of the jump rounds (all of them, with
 * the host's looks in between) and of the tally (with the table's initialisation and finish) of the last wdpm_catch_label. */
#define WDPM_CATCH_PHASES 3
int wdpm_catch_phase_ms(wdpm_ponds *h, double *ms /* WDPM_CATCH_PHASES values */);

#ifdef __cplusplus
}
#endif
#endif
