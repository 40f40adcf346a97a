/*
 * wdpm_ponds_priv.h — what the units of the pond inventory share: wdpm_ponds.hip (labels and table), wdpm_pond_rims.hip
 * (rims), wdpm_pond_catchments.hip (catchments), wdpm_pond_outlets.hip (outlets) and wdpm_pond_curves.hip (stage curves).  Geometry, the order-preserving image of a
 * double, the table rows as the device accumulates them, the wave helpers of the kernels (a lane's neighbour, the wave's extremum,
 * the look before an atomic) and - outside the host emulations of the tests, which define WDPM_PONDS_EMULATION and bring stand-ins
 * for the HIP device language (tests/hip_emu.h) - the handle itself with its guarded allocator.  Private: nothing here is exported,
 * and no header under include/ knows it.
 */
#ifndef WDPM_PONDS_PRIV_H
#define WDPM_PONDS_PRIV_H

#ifndef WDPM_PONDS_EMULATION
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "wdpm_ctx.h"

#define HIP_TRY(expr)                                                                                  \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) return wdpm_fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)
#endif
#include <cstddef>

#include "../../include/wdpm_group_ponds.h"
#include "../../include/wdpm_pond_rims.h"
#include "../../include/wdpm_group_pond_rims.h"
#include "../../include/wdpm_pond_catchments.h"
#include "../../include/wdpm_pond_outlets.h"
#include "../../include/wdpm_group_pond_catchments.h"
#include "../../include/wdpm_group_pond_outlets.h"
#include "../../include/wdpm_pond_curves.h"

namespace wdpm_pond_detail {

constexpr int kSeg = 64;             /* columns per segment = lanes per wave */
constexpr int kBlock = 256;          /* threads per block: four waves, four segments */
constexpr int kWaves = kBlock / kSeg;
constexpr int kTableWaves = 32768;   /* the table kernel aims at this many waves: bounds the atomics on one table row */

/* Rows one wave of the table kernel (and of the rim kernels) owns: about kTableWaves waves whatever the raster's size, or what
 * the caller forces (WDPM_PONDS_ROWS_PER_WAVE when the handle is made: tests and tuning).  The host and the host emulations both
 * ask here. */
constexpr int ponds_rows_per_wave(long long nseg, int rows, int forced) {
  long long rpw = forced > 0 ? forced : (nseg + kTableWaves - 1) / kTableWaves;
  if (rpw < 1) rpw = 1;
  if (rpw > rows) rpw = rows;
  return (int)rpw;
}

/* the table as the device accumulates it: wdpm_pond with the depth as its order-preserving image */
struct PondRow {
  int first_row, first_col;
  unsigned long long cells;
  unsigned long long volume_q;
  unsigned long long depth_key;
  int row_min, row_max, col_min, col_max;
};
static_assert(sizeof(PondRow) == sizeof(wdpm_pond), "the device table is copied out as wdpm_pond");

/* the rim table as the device accumulates it: wdpm_pond_rim with its three doubles as their order-preserving images and the rim
 * cell as a view-local padded index (INT_MAX: none yet) */
struct RimRow {
  unsigned long long smin_key, smax_key, rim_key;
  int rim_idx, pad;
  unsigned long long rim_cells, wall_cells;
};
static_assert(sizeof(RimRow) == sizeof(wdpm_pond_rim), "the device rim table is copied out as wdpm_pond_rim");

/* the catchment table as the device accumulates it: wdpm_pond_catchment with the head level as its order-preserving image */
struct CatchRow {
  unsigned long long catch_cells, inflow_cells, head_key;
  int row_min, row_max, col_min, col_max;
};
static_assert(sizeof(CatchRow) == sizeof(wdpm_pond_catchment) && sizeof(CatchRow) == 40, "the device catchment table is copied out as wdpm_pond_catchment");

/* Pointer jumping over the link raster runs in rounds, each of which at least halves every descent: 32 would do for fewer than
 * 2^31 cells.  Past kCatchRoundCap the call fails; the host looks at the count of unresolved cells once per kCatchBatch rounds. */
constexpr int kCatchRoundCap = 40;
constexpr int kCatchBatch = 4;
constexpr int kCatchHops = 4;        /* links one thread follows in one round */
constexpr int kCatchEvents = 6;      /* HIP events a handle keeps for the catchment phases */
static_assert(kCatchRoundCap % kCatchBatch == 0, "whole batches up to the cap");

/* what the catchment kernels count for the host: unres[k] is the number of cells round k left with a link that is no terminal */
struct CatchStatus {
  unsigned long long slope, pit, unponded;
  unsigned unres[kCatchRoundCap];
  unsigned long long exits;          /* row blocks: owned cells whose link was an exit when the tally met it */
};

/* the outlet table as the device accumulates it: wdpm_pond_outlet with the pour level as its order-preserving image (~0: no pass
 * yet) and the outlet pair as from_index * 8 + direction in the place of the four coordinates (~0: none yet) */
struct OutletRow {
  unsigned long long pour_key, pair, spare;
  int to_basin, reserved;
  unsigned long long divide_cells, fill_cells, fill_q;
};
static_assert(sizeof(OutletRow) == sizeof(wdpm_pond_outlet) && sizeof(OutletRow) == 56, "the device outlet table is copied out as wdpm_pond_outlet");
static_assert(offsetof(wdpm_pond_outlet, from_row) == offsetof(OutletRow, pair) && offsetof(wdpm_pond_outlet, to_basin) == offsetof(OutletRow, to_basin) &&
              offsetof(wdpm_pond_outlet, divide_cells) == offsetof(OutletRow, divide_cells) && offsetof(wdpm_pond_outlet, fill_q) == offsetof(OutletRow, fill_q),
              "the finish kernel rewrites a row in place");

/* what the outlet kernels count for the host */
struct OutletStatus {
  unsigned long long no_outlet, to_land, divide;
  unsigned deep;           /* a fill term of >= 512 m, or one that is not finite */
  unsigned pad;
};

/* the curve table as the device accumulates it: wdpm_pond_curve with the bed level as its order-preserving image (~0: no cell yet);
 * the top level is a double from the start (the outlet table's finished pour_level) */
struct CurveRow {
  unsigned long long bed_key;
  double top_level;
  unsigned long long cells[WDPM_CURVE_STAGES], q[WDPM_CURVE_STAGES];
};
static_assert(sizeof(CurveRow) == sizeof(wdpm_pond_curve) && sizeof(CurveRow) == 272, "the device curve table is copied out as wdpm_pond_curve");
static_assert(offsetof(wdpm_pond_curve, top_level) == offsetof(CurveRow, top_level) && offsetof(wdpm_pond_curve, cells) == offsetof(CurveRow, cells) &&
              offsetof(wdpm_pond_curve, q) == offsetof(CurveRow, q), "the finish kernel rewrites a row in place");
constexpr int kCurveWords = (int)(sizeof(CurveRow) / sizeof(unsigned long long));

/* what the curve kernels count for the host */
struct CurveStatus {
  unsigned long long no_curve, flat, stage_cells;
  unsigned deep;           /* a term of q of >= 512 m, or one that is not finite */
  unsigned pad;
};

/* status words the host reads after the scan */
struct Status {
  long long ponds;
  unsigned long long unions, seam_unions;
  unsigned deep;           /* a pond cell of >= 512 m */
  unsigned pad;
};

struct Geom {
  int rows, ncp, nsc;      /* padded rows, padded columns, segments per row */
  int nseg;                /* rows * nsc */
};

__device__ __forceinline__ unsigned long long depth_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double depth_from_key(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}
__device__ __forceinline__ int bit(unsigned long long m, int pos) { return (int)((m >> pos) & 1ull); }

/* the value of the lane to the left (right); lane 0 (63) takes `edge`, the cell beside the segment */
template <class T>
__device__ __forceinline__ T lane_from_left(T v, T edge, int lane) {
  const T t = __shfl_up(v, 1);
  return lane > 0 ? t : edge;
}
template <class T>
__device__ __forceinline__ T lane_from_right(T v, T edge, int lane) {
  const T t = __shfl_down(v, 1);
  return lane < 63 ? t : edge;
}

/* butterflies: every lane ends with the wave's extremum */
__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long t = __shfl_xor(v, d);
    v = t < v ? t : v;
  }
  return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long t = __shfl_xor(v, d);
    v = t > v ? t : v;
  }
  return v;
}

/* A table's extrema only move one way, so a look first spares the atomic that would change nothing; what a carry never gathered
 * still holds its start value and passes no look. */
template <class T>
__device__ __forceinline__ void atomic_min_if(T *p, T v) {
  if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > v) atomicMin(p, v);
}
template <class T>
__device__ __forceinline__ void atomic_max_if(T *p, T v) {
  if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v) atomicMax(p, v);
}

#ifndef WDPM_PONDS_EMULATION
struct Guarded { char *base; size_t bytes; };
/* blocks of a launch with per_block items each (the host emulations bring their own with their launch) */
inline unsigned blocks_for(long long items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }
#endif

}  // namespace wdpm_pond_detail

#ifndef WDPM_PONDS_EMULATION
/* The handle labels a VIEW of its context: rows [row_off, row_off + g.rows) of the context's rasters, whose first and last row the
 * kernels take for the dry border.  wdpm_ponds_create views a whole-raster context; a row block of a group (wdpm_group_ponds_*) is
 * viewed as its owned rows with one row either side. */
struct wdpm_ponds {
  wdpm_ctx *x;
  wdpm_pond_detail::Geom g;
  int row_off;                      /* context row of the view's row 0 */
  bool seams;                       /* a row block: the labels of rows 1 and g.rows - 2 come to the host with the status */
  size_t guard;                     /* bytes of each guard band (WDPM_GUARD_KB when the handle was made) */
  std::vector<wdpm_pond_detail::Guarded> guards;
  bool allocated;
  unsigned long long *d_masks, *d_rootmask, *d_busum;
  int *d_parent, *d_labels, *d_cnt, *d_bsum;
  unsigned *d_ucnt;
  wdpm_pond_detail::Status *d_status, *h_status;      /* h_status pinned */
  int *d_seam, *h_seam;             /* 2 x g.ncp labels (seams); h_seam pinned */
  int *d_map;                       /* local label - 1 -> label in the whole raster (seams) */
  long long map_cap;
  int *h_map;                       /* pinned staging (seams): the map on its way up, the finished table on its way down - */
  wdpm_pond *h_table;               /* a copy to or from pageable memory would make the host wait inside the queueing step */
  long long stage_cap;
  wdpm_pond_detail::PondRow *d_table;
  long long table_cap;
  int nb;                           /* blocks of the scan */
  int forced_rpw;                   /* WDPM_PONDS_ROWS_PER_WAVE when the handle was made, 0: the library chooses */
  int rpw;                          /* of the call under way */
  wdpm_pond_detail::Status last;    /* status words of the call under way */
  bool valid;                       /* the last label call succeeded */
  bool timing;                      /* WDPM_PONDS_TIMING=1 when the handle was made: HIP events around every kernel */
  hipEvent_t ev[WDPM_PONDS_PHASES + 2];   /* the host reads the status between scan and table: two marks there */
  double phase_ms[WDPM_PONDS_PHASES];
  wdpm_pond_stats stats;
  /* rims (wdpm_pond_rims.hip): the table of the last wdpm_rims_label; every label call takes rims_valid away first */
  wdpm_pond_detail::RimRow *d_rims;
  long long rims_cap;
  bool rims_valid;
  hipEvent_t rim_ev[WDPM_RIMS_PHASES + 1];   /* made with the others when the handle records events */
  double rim_ms[WDPM_RIMS_PHASES];
  /* rims of a row block (wdpm_group_rims_label): d_rims then holds one row per SLOT - the rank's local ponds, then its foreign
   * ponds - and d_slot_of[label in the whole raster] says which */
  int *d_slot_of;
  long long slot_cap;               /* entries of d_slot_of */
  int *d_foreign;                   /* 2 x g.ncp: the foreign ponds' labels */
  unsigned long long *h_beside;     /* pinned staging: 2 x g.nsc wet masks, 2 x g.ncp labels of the rows beside the rank's own, */
                                    /* 2 x g.ncp foreign labels */
  wdpm_pond_rim *h_rims;            /* pinned: the finished rim rows on their way down */
  long long h_rims_cap;
  long long rim_slots;              /* of the call under way */
  long long rim_foreign;
  std::vector<int> slot_label;      /* slot -> label in the whole raster */
  /* catchments (wdpm_pond_catchments.hip): link raster (the basin raster once a call has ended) and table of the last
   * wdpm_catch_label; every label call takes catch_valid away first */
  int *d_link;                      /* g.rows x g.ncp, allocated at the first wdpm_catch_label */
  wdpm_pond_detail::CatchRow *d_catch;
  long long catch_cap;
  wdpm_pond_detail::CatchStatus *d_cstat, *h_cstat;   /* h_cstat pinned */
  bool catch_valid;
  hipEvent_t catch_ev[wdpm_pond_detail::kCatchEvents];   /* init | receivers | jump rounds | tally, finish; row blocks: 0-1 receivers, 2-3 a batch of */
                                    /* jump rounds, 4-5 tally */
  double catch_ms[WDPM_CATCH_PHASES];
  wdpm_pond_catchment_stats catch_stats;
  /* catchments of a row block (wdpm_group_catch_label): d_catch then holds one row per SLOT - the rims' slots, then the rank's
   * remote ponds - and d_link's rows 0 and g.rows - 1 belong to the neighbours */
  unsigned long long *d_ckeys;      /* 4 x g.ncp level keys: the rank's first and last owned row, then the rows beside them */
  unsigned long long *h_ckeys;      /* pinned, laid out likewise: two rows on their way down, two on their way up */
  int *d_cexit;                     /* 4 x g.ncp: where each exit ends (2 x g.ncp), the remote ponds' labels */
  int *h_cexit;                     /* pinned, 6 x g.ncp: the links of the first and last owned row on their way down (and, behind the */
                                    /* tally, the same rows as basins: the seam basins of the outlet pass), then as d_cexit */
  wdpm_pond_catchment *h_catch;     /* pinned: the finished catchment rows on their way down */
  long long h_catch_cap;
  long long catch_slots, catch_remote;   /* of the call under way */
  int catch_rounds;
  std::vector<int> catch_remote_label;   /* the whole-raster labels of the remote slots, which follow the rims' slots (slot_label) */
  /* outlets (wdpm_pond_outlets.hip): the table of the last wdpm_outlets_label; every label call takes outlets_valid away first */
  wdpm_pond_detail::OutletRow *d_outlets;
  long long outlets_cap;
  wdpm_pond_detail::OutletStatus *d_ostat, *h_ostat;  /* h_ostat pinned */
  bool outlets_valid;
  hipEvent_t outlet_ev[WDPM_OUTLETS_PHASES + 1];      /* init, passes | locate, finish */
  double outlet_ms[WDPM_OUTLETS_PHASES];
  wdpm_pond_outlet_stats outlet_stats;
  /* outlets of a row block (wdpm_group_outlets_label): d_outlets then holds one row per SLOT, as d_catch does */
  unsigned long long *d_okeys;      /* 2 x okeys_cap: every slot's pour key and divide count on their way down, the merged keys on their way up */
  unsigned long long *h_okeys;      /* pinned, 3 x okeys_cap: keys and counts as they came down, then the merged keys */
  long long okeys_cap;
  wdpm_pond_detail::OutletRow *h_outlets;   /* pinned: the slots' rows on their way down */
  long long h_outlets_cap;
  int *h_oseam;                     /* pinned, 2 x g.ncp: the facing ranks' seam basins on their way up */
  /* stage curves (wdpm_pond_curves.hip): the table of the last wdpm_curves_label; every label call takes curves_valid away first */
  wdpm_pond_detail::CurveRow *d_curves;
  long long curves_cap;
  wdpm_pond_detail::CurveStatus *d_vstat, *h_vstat;   /* h_vstat pinned */
  bool curves_valid;
  hipEvent_t curve_ev[WDPM_CURVES_PHASES + 1];        /* init, bed | stages, finish */
  double curve_ms[WDPM_CURVES_PHASES];
  wdpm_pond_curve_stats curve_stats;
};

/* the handle of include/wdpm_group_ponds.h, include/wdpm_group_pond_rims.h, include/wdpm_group_pond_catchments.h and
 * include/wdpm_group_pond_outlets.h */
struct wdpm_group_ponds {
  wdpm_group *grp;
  int n;                                   /* ranks */
  int rows, ncp;                           /* the whole raster, padded */
  std::vector<wdpm_ponds *> r;             /* one handle per rank, on its owned rows with one row either side */
  std::vector<int> own_lo, own_rows, view0;   /* whole-raster rows: first owned, how many owned, the view's row 0 */
  std::vector<wdpm_pond> table;            /* the merged table of the last label call */
  bool timing, valid;
  wdpm_group_pond_stats stats;
  /* rims: the merged table of the last wdpm_group_rims_label; every label call takes rims_valid away first */
  std::vector<wdpm_pond_rim> rims;
  bool rims_valid;
  wdpm_group_rim_stats rim_stats;
  /* catchments: the merged table of the last wdpm_group_catch_label; every label call takes catch_valid away first */
  std::vector<wdpm_pond_catchment> catchments;
  bool catch_valid;
  wdpm_group_catchment_stats catch_stats;
  /* outlets: the merged table of the last wdpm_group_outlets_label; every label call takes outlets_valid away first */
  std::vector<wdpm_pond_outlet> outlets;
  bool outlets_valid;
  wdpm_group_outlet_stats outlet_stats;
};

namespace wdpm_pond_detail {
/* device memory of the handle between two guard bands (when it carries any): wdpm_ponds_guard_bad looks at every band */
__attribute__((visibility("hidden"))) hipError_t guarded_malloc(wdpm_ponds *h, void **p, size_t bytes);
__attribute__((visibility("hidden"))) void guarded_free(wdpm_ponds *h, void *p);
/* wdpm_group_ponds_label, and with `rims` what wdpm_group_rims_label adds to it: after rank i's table kernels are queued and
 * before any rank is waited for, rims(h, i, map) queues that rank's rim work, map[rank][local label - 1] being the stitch's
 * numbers.  One wait per rank then ends both. */
typedef int (*group_rims_queue)(wdpm_group_ponds *h, int rank, const std::vector<std::vector<int>> &map, long long ponds);
/* `seams` (may be null): called for rank i right after its scan is queued and before any rank is waited for, so that what it
 * sends to the host arrives with the seam labels. */
typedef int (*group_seams_queue)(wdpm_group_ponds *h, int rank);
__attribute__((visibility("hidden"))) int group_label(wdpm_group_ponds *h, double min_depth, int64_t *nponds, group_rims_queue rims,
                                                      group_seams_queue seams = nullptr);
/* wdpm_pond_rims.hip: the rims argument of wdpm_group_rims_label, and what that call does once group_label has returned - the
 * ranks' rim rows merged into h->rims, h->valid and h->rims_valid set.  wdpm_group_catch_label runs both and adds its own. */
__attribute__((visibility("hidden"))) int group_rims_rank(wdpm_group_ponds *h, int rank, const std::vector<std::vector<int>> &map, long long ponds);
__attribute__((visibility("hidden"))) int group_rims_merge(wdpm_group_ponds *h, const char *caller, long long ponds);
}  // namespace wdpm_pond_detail
#endif

#endif
