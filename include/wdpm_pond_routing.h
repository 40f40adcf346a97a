/*
 * wdpm_pond_routing.h — a runoff depth sent down the spill graph (include/wdpm_pond_spills.h): if r metres of runoff fall on every
 * basin, which ponds fill, how much each passes on, how much leaves over land or at a ring, and what land is connected to each pond
 * afterwards - one point of the contributing-area-against-runoff curve of the fill-and-spill literature.  One table row per pond.
 * Product library only, conventions as in wdpm_pond_spills.h.  The water of the context is not changed.
 *
 * Definitions (exact: every result is an integer, bit-reproducible whatever order the device visits the ponds in).  Ponds are 1..N of
 * a wdpm_spill_label; next, hops, fill_q, cells and catch_cells are that call's.
 *   runoff_q     rint(runoff_m * 2^24) (wdpm_route_runoff_q): runoff_m finite and >= 0, runoff_q < 2^32 (256 m)
 *   area(k)      cells + catch_cells of pond k;  own_q(k) = runoff_q * area(k).  A context holds < 2^31 cells and basins are
 *                disjoint, so no sum below leaves 64 bits
 *   in_q(k)      the sum of out_q(u) over the ponds u with next(u) == k.  next is the spill table's, ring heads cut: a head's
 *                overflow does not enter its successor
 *   out_q(k)     0 where next(k) == -1 (no outlet: the pond keeps everything); otherwise max(0, own_q + in_q - fill_q)
 *   kept_q       own_q + in_q - out_q
 *   overflows    out_q > 0
 *   full         next != -1 and own_q + in_q >= fill_q: a pond can be full without overflowing
 *   level        hops(k): the ponds of one level are independent of each other, and a pond spills into the level below its own
 *   reach_ponds, reach_cells
 *                sums of 1 and of area(u) over k itself and the ponds u upstream of k along next > 0 for which every pond from u up
 *                to, but not including, k overflows: the land connected to k after the event
 * Overflow is max(0, ...), not a sum: the ponds are taken level by level, the deepest first.
 */
#ifndef WDPM_POND_ROUTING_H
#define WDPM_POND_ROUTING_H

#include "wdpm_pond_spills.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one table row: pond k is row k - 1; 64 bytes */
typedef struct wdpm_pond_route {
  uint64_t own_q, in_q, kept_q, out_q;
  int64_t  reach_ponds, reach_cells;
  int32_t  overflows, full, level, reserved;
} wdpm_pond_route;

/* of the last wdpm_route_label or wdpm_route_rerun.  own_q == kept_q + out_land_q + out_ring_q, summed over all ponds */
typedef struct wdpm_pond_route_stats {
  int64_t  ponds;
  int64_t  runoff_q;
  int64_t  levels;            /* max_hops + 1; 0 without a pond */
  int64_t  wide_levels;       /* levels of more ponds than one workgroup: a grid launch each */
  int64_t  launches;          /* of the sweep: the wide levels and the runs of narrow ones */
  int64_t  overflowing;
  int64_t  full;
  uint64_t own_q, kept_q;
  uint64_t out_land_q;        /* out of ponds with next == 0 */
  uint64_t out_ring_q;        /* out of ring heads (next == -2) */
} wdpm_pond_route_stats;

/* rint(runoff_m * 2^24), or -1 where wdpm_route_label refuses runoff_m: not finite, negative, or 2^32 quanta and more.  Pure. */
int64_t wdpm_route_runoff_q(double runoff_m);

/* wdpm_spill_label, then the routing pass on the tables it left, on the same stream: every older query, wdpm_spill_* included,
 * answers as after wdpm_spill_label.  Any lesser label call - wdpm_ponds_label up to wdpm_spill_label - takes the routing table
 * away.  Handles of wdpm_ponds_create only.  A call that fails leaves the handle without any table; the handle itself stays usable. */
int wdpm_route_label(wdpm_ponds *h, double min_depth, double headroom_tol, double runoff_m, int64_t *nponds);
/* Another runoff depth on what the last successful wdpm_route_label left - the ponds in level order, the launches, the gathered
 * tables: sweep and finish only, nothing is labelled again.  Fails without that state; a refused runoff_m leaves every table in
 * place. */
int wdpm_route_rerun(wdpm_ponds *h, double runoff_m);
/* the routing table of the last wdpm_route_label or wdpm_route_rerun: N rows; capacity < N fails and writes nothing */
int wdpm_route_table(wdpm_ponds *h, wdpm_pond_route *out, int64_t capacity);
int wdpm_route_stats(wdpm_ponds *h, wdpm_pond_route_stats *out);
/* With WDPM_PONDS_TIMING=1 set when the handle was made: milliseconds of the ordering of the ponds by level (0 after a rerun), of
 * the sweep and of the finish of the last wdpm_route_label or wdpm_route_rerun.
 * Read when the handle is made, for tests and tuning: WDPM_ROUTE_NARROW=n (1 <= n <= 256), the most ponds a level may hold and still
 * be walked inside a run; WDPM_ROUTE_RUN_LEVELS=m (>= 1, default 65536), the most levels to a run. */
#define WDPM_ROUTE_PHASES 3
int wdpm_route_phase_ms(wdpm_ponds *h, double *ms /* WDPM_ROUTE_PHASES values */);

#ifdef __cplusplus
}
#endif
#endif
