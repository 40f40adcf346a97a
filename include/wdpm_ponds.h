/*
 * wdpm_ponds.h — pond inventory of a context's current water raster (product library only).
 *
 * A second header beside wdpm.h: the CPU restatement used by the tests exports wdpm.h alone, so
 * nothing here is part of that ABI.  Conventions as in wdpm.h: plain C, every function returns 0 on
 * success and non-zero on failure, wdpm_last_error() then returns a message.
 *
 * Definitions (exact: every result below is an integer or an exact double, and no result depends on
 * the order in which the device visits the cells)
 *   pond cell   dem < +inf && w > min_depth (strict), on the context's current water raster with the
 *               owed threshold flush and the owed drain() applied; NaN depths, NODATA cells and the
 *               one-cell border never are pond cells
 *   pond        a maximal 8-connected set of pond cells
 *   first cell  the pond's smallest padded row-major index; ponds are numbered 1..N by first cell
 *   labels      int32, padded layout rows x (ncols + 2): 0 = no pond, k = pond k
 *   volume_q    sum over the pond of rint(w * 2^24), round half to even; volume_q * 2^-24 is the
 *               volume in metres x cells.  Cannot overflow below 512 m of depth: a pond cell of
 *               >= 512 m (or +inf) fails wdpm_ponds_label with a message.
 */
#ifndef WDPM_PONDS_H
#define WDPM_PONDS_H

#include "wdpm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wdpm_ponds wdpm_ponds; /* opaque */

/* one table row: pond k is row k - 1.  Coordinates are padded (file coordinate + 1). */
typedef struct wdpm_pond {
  int32_t  first_row, first_col;
  int64_t  cells;
  uint64_t volume_q;
  double   max_depth;
  int32_t  row_min, row_max, col_min, col_max;
} wdpm_pond;

/* what the last wdpm_ponds_label did */
typedef struct wdpm_pond_stats {
  int64_t segments;       /* work items of the run kernels: 64-column row segments, one wave each */
  int64_t unions;         /* unions made, one per pair of touching runs (row seams and column seams) */
  int64_t seam_unions;    /* of those, the ones across a 64-column segment seam (straight or diagonal) */
  int64_t passes;         /* passes of iterate-until-stable steps: this design has none, always 0 */
  int64_t rows_per_wave;  /* rows one wave of the table kernel reduces before its atomics go out */
  int64_t ponds;          /* N of that call */
} wdpm_pond_stats;

/* Whole-raster contexts only (a slab context is refused).  Reads the context through its own stream; never changes
 * what an iteration launch reads.  With WDPM_GUARD_KB set when the handle is made its device buffers carry guard bands.
 * WDPM_PONDS_ROWS_PER_WAVE=n, read at the same moment, fixes how many rows a wave of the table kernel reduces before its atomics
 * go out (tests, tuning; default: chosen from the raster's size).  Destroy the handle before its context. */
int  wdpm_ponds_create(wdpm_ponds **out, wdpm_ctx *ctx);
void wdpm_ponds_destroy(wdpm_ponds *h);
/* label, number and accumulate; min_depth finite and >= 0 (metres) */
int  wdpm_ponds_label(wdpm_ponds *h, double min_depth, int64_t *nponds);
/* the table of the last label call: N rows; capacity < N fails and writes nothing */
int  wdpm_ponds_table(wdpm_ponds *h, wdpm_pond *out, int64_t capacity);
/* the label raster of the last label call: rows x (ncols + 2) int32 */
int  wdpm_ponds_labels(wdpm_ponds *h, int32_t *padded);
/* guard bytes around the handle's device buffers that no longer hold their fill (0 without WDPM_GUARD_KB) */
int  wdpm_ponds_guard_bad(wdpm_ponds *h, int64_t *bytes);
int  wdpm_ponds_stats(wdpm_ponds *h, wdpm_pond_stats *out);
/* With WDPM_PONDS_TIMING=1 set when the handle is made, HIP events bracket the kernels of every label call: milliseconds of
 * mask, merge, flatten, scan, table (with its initialisation) and finish of the last one.  Fails on a handle made without it. */
#define WDPM_PONDS_PHASES 6
int  wdpm_ponds_phase_ms(wdpm_ponds *h, double *ms /* WDPM_PONDS_PHASES values */);

#ifdef __cplusplus
}
#endif
#endif
