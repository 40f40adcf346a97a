/*
 * wdpm_group_pond_curves.h — the stage curve of every pond of a raster spread over the row blocks of a wdpm_group: the table of
 * wdpm_pond_curves.h, taken where the rows lie.  Product library only.  A ninth header, on the handle of wdpm_group_ponds.h.
 *
 * Definitions and the 272-byte table row are those of wdpm_pond_curves.h, unchanged: bed_level, top_level, the stage heights by the
 * rule of wdpm_curves_stage_level, cells, q.  The result equals, value for value (bed_level and top_level bit for bit), what
 * wdpm_curves_table and wdpm_curves_stats give on a whole-raster context that holds the water wdpm_group_download_water returns.  No
 * water, label or basin raster comes to the host for it, and there is no second context.
 *
 * Who computes what.  Neither curve pass has a stencil: a rank walks its owned rows and never reads a row beyond them.  But the bed of
 * a basin is the lowest ground over ALL ranks, and every stage height depends on it, so the host stands between the two device
 * passes: the ranks' own lowest ground per basin comes down (8 bytes per slot, still the order-preserving image of a double), the
 * lowest per pond goes back up, and then every rank - whether it holds the bed or not - forms the same sixteen heights and counts its
 * own cells against them.  The top level is the pour level wdpm_group_outlets_label merged over all ranks, as that call left it on
 * each device.  The host adds the ranks' rows up and turns the bed key into a double, once per pond.
 *
 * Scope: the ranks of ONE process, as wdpm_group_ponds.h.  A group of one rank runs the same path and gives the single-context answer.
 */
#ifndef WDPM_GROUP_POND_CURVES_H
#define WDPM_GROUP_POND_CURVES_H

#include "wdpm_group_pond_outlets.h"
#include "wdpm_pond_curves.h"

#ifdef __cplusplus
extern "C" {
#endif

/* of the last wdpm_group_curves_label: the four counts of wdpm_pond_curve_stats for the whole raster, then the group's own */
typedef struct wdpm_group_curve_stats {
  int64_t ponds;
  int64_t no_curve;
  int64_t flat;
  int64_t stage_cells;
  int64_t ranks;             /* row blocks */
  int64_t split_basins;      /* ponds for which more than one rank offered a bed key */
  int64_t remote_beds;       /* ponds that have stage cells on a rank other than the lowest rank holding the bed */
  double  merge_ms;          /* host time of both merges, milliseconds */
} wdpm_group_curve_stats;

/* wdpm_group_outlets_label, and the curve passes of every rank on the same water, from one call.  Afterwards every older
 * wdpm_group_* query answers exactly as after wdpm_group_outlets_label.  A later wdpm_group_ponds_label, wdpm_group_rims_label,
 * wdpm_group_catch_label or wdpm_group_outlets_label takes the curve table away.  A call that fails - as those calls fail, over a term
 * of q of 512 m or more or one that is not finite on any rank, over memory, over a device error, over a sum that leaves 64 bits -
 * leaves the handle without any table; the handle itself stays usable. */
int wdpm_group_curves_label(wdpm_group_ponds *h, double min_depth, int64_t *nponds);
/* the curve table of the last wdpm_group_curves_label: N rows; capacity < N fails and writes nothing */
int wdpm_group_curves_table(wdpm_group_ponds *h, wdpm_pond_curve *out, int64_t capacity);
int wdpm_group_curves_stats(wdpm_group_ponds *h, wdpm_group_curve_stats *out);
/* WDPM_CURVES_PHASES values for one rank, as wdpm_curves_phase_ms: "bed" is the table's initialisation, the bed pass and the keys laid
 * side by side, "stages" the merged keys on their way up and the stage pass; fails on a handle made without WDPM_PONDS_TIMING=1.  The
 * host's time is wdpm_group_curve_stats::merge_ms. */
int wdpm_group_curves_phase_ms(wdpm_group_ponds *h, int32_t rank, double *ms /* WDPM_CURVES_PHASES values */);

#ifdef __cplusplus
}
#endif
#endif
