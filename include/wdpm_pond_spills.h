/*
 * wdpm_pond_spills.h — where the overflow of every pond of the inventory (include/wdpm_ponds.h) ends up: the graph the outlet table
 * (include/wdpm_pond_outlets.h) spans with its to_basin column, followed downstream pond by pond.  Per pond the end of its chain and
 * the storage on the way, the land and the ponds that drain through it once everything above it is full, and the part of both that
 * is connected to it now, through ponds that already stand at their pour level - the contributing area of the fill-and-spill
 * literature.  One table row per pond.  Product library only, conventions as in wdpm_pond_curves.h.
 *
 * Definitions (exact: every result is an integer, bit-reproducible whatever order the device visits the ponds in).  The inputs are
 * the tables a wdpm_curves_label leaves for ponds 1..N: cells of wdpm_pond, surface_max of wdpm_pond_rim, catch_cells of
 * wdpm_pond_catchment, and pour_level, to_basin and fill_q of wdpm_pond_outlet.
 *   spilling(k)  pond k has an outlet (to_basin >= 0) and pour_level - surface_max <= headroom_tol: one fp64 subtraction, compared as
 *                doubles.  headroom_tol is a parameter of the label call, finite and >= 0; with 0 the surface stands at or above
 *                the pour level
 *   ring         ponds k1 -> k2 -> ... -> km -> k1 along to_basin, m >= 2 (a pond never spills into itself).  A pass between two
 *                basins is a pass of both, so the pour level never rises along to_basin, and all m pour levels of a ring are equal.
 *                A mutual pair is the common case; three or more need tied passes.  The ring's HEAD is its smallest label
 *   next(k)      to_basin of pond k, except at a ring head, where it is -2.  So j > 0 is pond j, 0 land that ends in a pit, -1 no
 *                outlet, -2 a ring closed here.  With the heads cut the ponds form a forest
 *   sink(k)      the last pond reached from k along next > 0; k itself when next(k) <= 0
 *   end(k)       next(sink(k)): 0, -1 or -2
 *   hops(k)      the edges walked from k to sink(k)
 *   path_fill_q  the sum of fill_q over the ponds from k to sink(k), both included: the storage to fill before water that leaves k
 *                reaches the end of its chain (quanta of 2^-24 m, like fill_q)
 *   up_ponds, up_cells, up_fill_q
 *                sums over the ponds u whose chain passes through k, k included: of 1, of cells + catch_cells and of fill_q.  Basins
 *                are disjoint, so no sum leaves 64 bits
 *   rest(k)      the first pond on k's chain, k included, that is not spilling, or sink(k) if all of them spill: where k's overflow
 *                comes to rest now.  rest(k) == k when k does not spill.  rest_hops(k): the edges walked from k to rest(k)
 *   live_ponds, live_cells
 *                the up_ sums over those u only for which every pond from u up to, but not including, k is spilling; k itself
 *                always counts: the land connected to k now
 * Merging the ponds of a ring into one depression is not done here: a ring is reported (its head has next == -2) and cut there.
 */
#ifndef WDPM_POND_SPILLS_H
#define WDPM_POND_SPILLS_H

#include "wdpm_pond_curves.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one table row: pond k is row k - 1; 80 bytes */
typedef struct wdpm_pond_spill {
  int32_t  next, sink, end, hops, rest, rest_hops, spilling, reserved;
  uint64_t path_fill_q;
  int64_t  up_ponds, up_cells;
  uint64_t up_fill_q;
  int64_t  live_ponds, live_cells;
} wdpm_pond_spill;

/* of the last wdpm_spill_label */
typedef struct wdpm_pond_spill_stats {
  int64_t ponds;
  int64_t rings;             /* ring heads */
  int64_t ring_ponds;        /* ponds that lie on a ring */
  int64_t spilling;
  int64_t ends_land;         /* sinks with next == 0 */
  int64_t ends_none;         /* sinks with next == -1 */
  int64_t ends_ring;         /* sinks with next == -2: equal to rings */
  int64_t max_hops;
  int64_t rounds;            /* launches of doubling kernels: 3 (ceil(log2 N) + 1), whatever the graph; 0 without a pond */
} wdpm_pond_spill_stats;

/* wdpm_curves_label, then the spill pass on the tables it left, queued on the context's stream with nothing in between: every older
 * query answers as after wdpm_curves_label.  Any lesser label call - wdpm_ponds_label up to wdpm_curves_label - takes the spill table
 * away.  Handles of wdpm_ponds_create only.  A call that fails leaves the handle without any table; the handle itself stays usable. */
int wdpm_spill_label(wdpm_ponds *h, double min_depth, double headroom_tol, int64_t *nponds);
/* the spill table of the last wdpm_spill_label: N rows; capacity < N fails and writes nothing */
int wdpm_spill_table(wdpm_ponds *h, wdpm_pond_spill *out, int64_t capacity);
int wdpm_spill_stats(wdpm_ponds *h, wdpm_pond_spill_stats *out);
/* With WDPM_PONDS_TIMING=1 set when the handle was made: milliseconds of the ring pass (with the gathering of the tables and the cut),
 * of the chain pass and of the sums (with the finish) of the last wdpm_spill_label. */
#define WDPM_SPILL_PHASES 3
int wdpm_spill_phase_ms(wdpm_ponds *h, double *ms /* WDPM_SPILL_PHASES values */);

#ifdef __cplusplus
}
#endif
#endif
