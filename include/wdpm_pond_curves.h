/*
 * wdpm_pond_curves.h — the stage curve of every pond of the inventory (include/wdpm_ponds.h): flooded area and storage of the pond's
 * basin (include/wdpm_pond_catchments.h) at sixteen levels between the lowest ground of the basin and the level at which it spills
 * (include/wdpm_pond_outlets.h).  wdpm_pond_outlet gives fill_cells and fill_q at the pour level only, above the water that stands
 * there now; this is the depression's whole stage-storage-area curve, whatever water stands in it.  One table row per pond.  Product
 * library only, conventions as in wdpm_ponds.h, wdpm_pond_rims.h, wdpm_pond_catchments.h and wdpm_pond_outlets.h.
 *
 * Definitions (exact: every result is an integer or an exact double, bit-reproducible whatever order the device visits the cells
 * in).  B is the basin raster of the call (wdpm_catch_basins), dem the elevation of a cell as the device holds it.  S = 16
 * (WDPM_CURVE_STAGES).  Doubles are compared through the order-preserving 64-bit image of a double the other units use (-0.0 below
 * +0.0).  For pond k (row k - 1):
 *   bed_level    Z: the lowest dem over the cells with B == k.  The DEM, not the level: the curve belongs to the depression,
 *                whatever water stands in it
 *   top_level    P: the pond's pour_level; +inf where the pond has no outlet
 *   stage height for P finite, h_s = Z + (P - Z) * (s / 16) for s = 1..15: exactly one fp64 subtraction, one fp64 multiplication by
 *                the exact constant s / 16 and one fp64 addition, each rounded to nearest, never a fused multiply-add; h_16 = P
 *                itself, not computed.  wdpm_curves_stage_level holds this rule, and the device uses the same three operations
 *   cells[s - 1] the number of cells c with B[c] == k and dem(c) STRICTLY below h_s
 *   q[s - 1]     the sum over those cells of rint((h_s - dem(c)) * 2^24): one fp64 subtraction per cell and stage, rounded half to
 *                even, in the quanta of wdpm_pond.volume_q and wdpm_pond_outlet.fill_q.  A term that is not finite or is 512 m or
 *                more fails the call with a message (the pond table's own bound; below it no sum of fewer than 2^31 terms leaves
 *                64 bits)
 * A pond without an outlet has top_level +inf and zeros in both arrays; its bed_level is still given.  A pond with P == Z has zeros.
 * cells and q are cumulative: both never fall from one stage to the next, and cells[15] >= fill_cells and q[15] >= fill_q of the same
 * pond, because dem <= level cell by cell and rint is monotone.
 */
#ifndef WDPM_POND_CURVES_H
#define WDPM_POND_CURVES_H

#include "wdpm_pond_outlets.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WDPM_CURVE_STAGES 16

/* one table row: pond k is row k - 1; 272 bytes; stage s is entry s - 1 */
typedef struct wdpm_pond_curve {
  double   bed_level, top_level;
  int64_t  cells[WDPM_CURVE_STAGES];
  uint64_t q[WDPM_CURVE_STAGES];
} wdpm_pond_curve;

/* of the last wdpm_curves_label */
typedef struct wdpm_pond_curve_stats {
  int64_t ponds;
  int64_t no_curve;          /* ponds without an outlet */
  int64_t flat;              /* ponds with top_level == bed_level */
  int64_t stage_cells;       /* cells[15] over all ponds */
} wdpm_pond_curve_stats;

/* wdpm_outlets_label, then the curve pass on the same water, queued on the context's stream with nothing in between: every older
 * query answers as after wdpm_outlets_label.  A later wdpm_ponds_label, wdpm_rims_label, wdpm_catch_label or wdpm_outlets_label takes
 * the curve table away.  Handles of wdpm_ponds_create only.  A call that fails - over a term of q, over memory, over a device error
 * - leaves the handle without any table, like a wdpm_outlets_label that fails over fill_q; the handle itself stays usable. */
int wdpm_curves_label(wdpm_ponds *h, double min_depth, int64_t *nponds);
/* the curve table of the last wdpm_curves_label: N rows; capacity < N fails and writes nothing */
int wdpm_curves_table(wdpm_ponds *h, wdpm_pond_curve *out, int64_t capacity);
int wdpm_curves_stats(wdpm_ponds *h, wdpm_pond_curve_stats *out);
/* With WDPM_PONDS_TIMING=1 set when the handle was made: milliseconds of the bed pass (with the table's initialisation) and of the
 * stage pass (with the finish) of the last wdpm_curves_label. */
#define WDPM_CURVES_PHASES 2
int wdpm_curves_phase_ms(wdpm_ponds *h, double *ms /* WDPM_CURVES_PHASES values */);
/* the stage rule: bed for s == 0, top for s == 16, bed + (top - bed) * (s / 16) in three rounded operations between them, NaN for
 * any other s.  Needs no handle and no device. */
double wdpm_curves_stage_level(double bed, double top, int s);

#ifdef __cplusplus
}
#endif
#endif
