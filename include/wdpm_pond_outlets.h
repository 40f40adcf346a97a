/*
 * wdpm_pond_outlets.h — the outlet of every pond of the inventory (include/wdpm_ponds.h): where its basin - the pond and its
 * catchment (include/wdpm_pond_catchments.h) - meets another basin at the lowest pass, how far the water is from there and what the
 * basin holds until it spills.  One table row per pond.  Product library only, conventions as in wdpm_ponds.h, wdpm_pond_rims.h and
 * wdpm_pond_catchments.h.
 *
 * Definitions (exact: every result is an integer or an exact double, bit-reproducible whatever order the device visits the cells
 * in).  B is the basin raster of the call (wdpm_catch_basins), `level` of a cell as in wdpm_pond_catchments.h.  Doubles are compared
 * through the order-preserving 64-bit image of a double that max_depth and rim_level use (-0.0 below +0.0).
 *   pass         of pond k: an ordered pair (a, b) of 8-neighbours with B[a] == k and B[b] >= 0, B[b] != k.  Its height is the
 *                larger of level(a) and level(b).  b may lie in basin 0 (land that ends in a pit); a cell with B == -1 (border,
 *                NODATA, NaN elevation) is a wall and forms no pass; a may be a pond cell or a cell of the catchment
 *   outlet       of pond k: its pass of lowest height; among equals the one whose a has the smallest padded row-major index, then
 *                the first b in neighbour order (up-left, up, up-right, left, right, down-left, down, down-right)
 *   pour_level   the outlet's height.  Never below the pond's rim_level (the lowest shore cell usually drains straight back)
 *   divide_cells the cells a of basin k that stand in at least one pass, each once
 *   fill_cells   the cells c with B[c] == k and level(c) STRICTLY below pour_level, pond cells included: the flooded area when the
 *                pond is about to spill.  Every such cell reaches the pond through lower cells of its own descent
 *   fill_q       the sum over those cells of rint((pour_level - level(c)) * 2^24): one fp64 subtraction per cell, rounded half to
 *                even, in the quanta of wdpm_pond.volume_q - the storage left until the spill.  A term that is not finite or is
 *                512 m or more fails the call with a message (the pond table's own bound)
 * A pond without any pass - one basin over the whole raster, a basin walled in - has pour_level +inf, coordinates -1,
 * to_basin -1 and zeros for the three counts.
 * For every call:  pour_level >= rim_level of the same pond wherever there is an outlet; and to_basin == j > 0 implies
 * pour_level of pond j <= pour_level of pond k, because the reversed pair is a pass of j.
 */
#ifndef WDPM_POND_OUTLETS_H
#define WDPM_POND_OUTLETS_H

#include "wdpm_pond_catchments.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one table row: pond k is row k - 1; 56 bytes; coordinates are padded */
typedef struct wdpm_pond_outlet {
  double   pour_level;
  int32_t  from_row, from_col, to_row, to_col;   /* a and b */
  int32_t  to_basin, reserved;                   /* B[b]: j > 0 a pond, 0 land that ends in a pit, -1 none; reserved = 0 */
  int64_t  divide_cells, fill_cells;
  uint64_t fill_q;
} wdpm_pond_outlet;

/* of the last wdpm_outlets_label */
typedef struct wdpm_pond_outlet_stats {
  int64_t ponds;
  int64_t no_outlet;         /* ponds without any pass */
  int64_t to_land;           /* ponds whose outlet leads to basin 0 */
  int64_t divide_cells;      /* over all ponds */
} wdpm_pond_outlet_stats;

/* wdpm_catch_label, then the outlet pass on the same water, queued on the context's stream with nothing in between: labels, pond
 * table, rim table, catchment table, basin raster and outlet table belong to the same water, and wdpm_ponds_*, wdpm_rims_table and
 * wdpm_catch_* answer as after wdpm_catch_label.  A later wdpm_ponds_label, wdpm_rims_label or wdpm_catch_label takes the outlet
 * table away.  Handles of wdpm_ponds_create only.  A call that fails - over fill_q, over memory, over a device error - leaves the
 * handle without any table, like a wdpm_ponds_label that fails over volume_q; the handle itself stays usable. */
int wdpm_outlets_label(wdpm_ponds *h, double min_depth, int64_t *nponds);
/* the outlet table of the last wdpm_outlets_label: N rows; capacity < N fails and writes nothing */
int wdpm_outlets_table(wdpm_ponds *h, wdpm_pond_outlet *out, int64_t capacity);
int wdpm_outlets_stats(wdpm_ponds *h, wdpm_pond_outlet_stats *out);
/* With WDPM_PONDS_TIMING=1 set when the handle was made: milliseconds of the pass over the pairs (with the table's initialisation)
 * and of the locate pass (with the fill sums and the finish) of the last wdpm_outlets_label. */
#define WDPM_OUTLETS_PHASES 2
int wdpm_outlets_phase_ms(wdpm_ponds *h, double *ms /* WDPM_OUTLETS_PHASES values */);

#ifdef __cplusplus
}
#endif
#endif
