/*
 * wdpm_ponds_priv.h — what the units of the pond inventory share: wdpm_ponds.hip (labels and table), wdpm_pond_rims.hip
 * (rims), wdpm_pond_catchments.hip (catchments), wdpm_pond_outlets.hip (outlets), wdpm_pond_curves.hip (stage curves), wdpm_pond_spills.hip (spills)
 * and wdpm_pond_routing.hip (routing).  Geometry, the order-preserving image of a
 * double, the table rows as the device accumulates them, the wave helpers of the kernels (a lane's neighbour, the wave's extremum,
 * the look before an atomic) and - outside the host emulations of the tests, which define WDPM_PONDS_EMULATION and bring stand-ins
 * for the HIP device language (tests/hip_emu.h) - the host side: the guarded allocator, the holders every buffer, status pair and
 * phase timer of the handle is made of, the handle as one record per unit, the row-block helpers and the one implementation of
 * each read-out ("The handle").  Private: nothing here is exported, and no header under include/ knows it.
 */
#ifndef WDPM_PONDS_PRIV_H
#define WDPM_PONDS_PRIV_H

#ifndef WDPM_PONDS_EMULATION
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <vector>

#include "wdpm_ctx.h"   /* the context, wdpm_fail, HIP_TRY */
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
#include "../../include/wdpm_group_pond_curves.h"
#include "../../include/wdpm_pond_spills.h"
#include "../../include/wdpm_pond_routing.h"
#include "wdpm_route_plan.h"

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

/* The spill passes (wdpm_pond_spills.hip) double pointers over the table of N < 2^31 ponds: R = ceil(log2 N) + 1 rounds per pass reach
 * 2^R >= 2 N steps, past any chain and twice round any ring.  The host and the host emulation both ask here. */
constexpr int kSpillMaxRounds = 32;
constexpr int kSpillPasses = 3;      /* rings, chains, sums */
constexpr int spill_rounds(long long n) {
  int r = 1;
  for (long long reach = 1; reach < n; reach <<= 1) r++;
  return r;
}

/* what the spill kernels count for the host, and what steers their rounds: work[pass][r] != 0 says that round r of the pass has
 * something to do; a round that finds 0 there returns at once, and so does every later one */
struct SpillStatus {
  unsigned long long rings, ring_ponds, spilling, ends_land, ends_none, ends_ring, max_hops;
  unsigned work[kSpillPasses][kSpillMaxRounds + 1];
  unsigned pad;
};

/* what the routing kernels (wdpm_pond_routing.hip) count for the host: the sweep the overflow that leaves the graph, the finish the
 * rest */
struct RouteStatus {
  unsigned long long overflowing, full, own_q, kept_q, out_land_q, out_ring_q;
};
static_assert(kRouteBlock == kBlock, "the planner's workgroup is the kernels'");

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

}  // namespace wdpm_pond_detail

#ifndef WDPM_PONDS_EMULATION
/* ---- host only: the handle, what it is made of, and what the units' entry points share -------------------------------------- */
#pragma GCC visibility push(hidden)
namespace wdpm_pond_detail {

struct Guarded { char *base; size_t bytes; };
/* blocks of a launch with per_block items each (the host emulations bring their own with their launch) */
inline unsigned blocks_for(long long items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

/* device memory of the handle between two guard bands (when it carries any): wdpm_ponds_guard_bad looks at every band */
hipError_t guarded_malloc(wdpm_ponds *h, void **p, size_t bytes);
void guarded_free(wdpm_ponds *h, void *p);

/* Holders.  Every buffer of the handle is one of these three, so that it starts empty, grows by one rule and is given back by one
 * reset(): DevBuf is guarded device memory, PinBuf pinned host memory, both with their capacity in elements. */
template <class T> struct DevBuf { T *p = nullptr; long long cap = 0; };
template <class T> struct PinBuf { T *p = nullptr; long long cap = 0; };
template <class T> void reset(wdpm_ponds *h, DevBuf<T> &b) { guarded_free(h, b.p); b.p = nullptr; b.cap = 0; }
template <class T> void reset(wdpm_ponds *, PinBuf<T> &b) { if (b.p) (void)hipHostFree(b.p); b.p = nullptr; b.cap = 0; }
/* Room for n elements: nothing when the buffer holds that many, else what it held is freed first (its contents are never wanted)
 * and on failure it is left empty.  A buffer of one fixed size is made by its first call. */
template <class T> hipError_t grow(wdpm_ponds *h, DevBuf<T> &b, long long n) {
  if (n <= b.cap) return hipSuccess;
  reset(h, b);
  const hipError_t e = guarded_malloc(h, (void **)&b.p, (size_t)n * sizeof(T));
  if (e == hipSuccess) b.cap = n; else b.p = nullptr;
  return e;
}
template <class T> hipError_t grow(wdpm_ponds *h, PinBuf<T> &b, long long n) {
  if (n <= b.cap) return hipSuccess;
  reset(h, b);
  const hipError_t e = hipHostMalloc(&b.p, (size_t)n * sizeof(T));
  if (e == hipSuccess) b.cap = n; else b.p = nullptr;
  return e;
}

/* the words a unit's kernels count for the host: one record on the device (no guard bands) and its pinned twin */
template <class T> struct StatusPair { T *d = nullptr, *h = nullptr; };
/* both at the first call, or neither; *what names the memory that ran out */
template <class T> hipError_t ensure(StatusPair<T> &s, const char **what) {
  if (s.d) return hipSuccess;
  *what = "device";
  hipError_t e = hipMalloc(&s.d, sizeof(T));
  if (e != hipSuccess) { s.d = nullptr; return e; }
  *what = "pinned host";
  e = hipHostMalloc(&s.h, sizeof(T));
  if (e != hipSuccess) { s.h = nullptr; (void)hipFree(s.d); s.d = nullptr; }
  return e;
}
template <class T> void reset(wdpm_ponds *, StatusPair<T> &s) {
  if (s.d) (void)hipFree(s.d);
  if (s.h) (void)hipHostFree(s.h);
  s.d = s.h = nullptr;
}

/* The HIP events of one unit and the milliseconds of its phases.  Which events bound which phase is the unit's business. */
template <int kEvents, int kPhases> struct PhaseTimer {
  static constexpr int phases = kPhases;
  hipEvent_t ev[kEvents] = {};
  double ms[kPhases] = {};
  /* when the handle records events; one that cannot be made ends the recording for the whole handle */
  void create(bool &timing) {
    for (int i = 0; timing && i < kEvents; i++)
      if (hipEventCreate(&ev[i]) != hipSuccess) timing = false;
  }
  void destroy() {
    for (hipEvent_t &e : ev) {
      if (e) (void)hipEventDestroy(e);
      e = nullptr;
    }
  }
  void clear() { for (double &m : ms) m = 0.0; }
  hipError_t mark(bool timing, int i, hipStream_t s) { return timing ? hipEventRecord(ev[i], s) : hipSuccess; }
  hipError_t read(int a, int b, double *out) {
    float f = 0.f;
    const hipError_t e = hipEventElapsedTime(&f, ev[a], ev[b]);
    *out = f;
    return e;
  }
  /* phase i lies between events i and i + 1 */
  hipError_t read_all() {
    hipError_t e = hipSuccess;
    for (int i = 0; i < kPhases && e == hipSuccess; i++) e = read(i, i + 1, &ms[i]);
    return e;
  }
};

/* One record per unit.  A row block's extra buffers lie in their unit's record; the whole-raster calls never touch them. */
struct LabelUnit {                  /* wdpm_ponds.hip: labels and pond table */
  bool allocated = false;           /* the buffers of one fixed size are there */
  DevBuf<unsigned long long> masks, rootmask, busum;
  DevBuf<int> parent, labels, cnt, bsum;
  DevBuf<unsigned> ucnt;
  StatusPair<Status> status;
  DevBuf<int> seam;                 /* 2 x g.ncp labels (row blocks) */
  PinBuf<int> h_seam;
  DevBuf<int> map;                  /* local label - 1 -> label in the whole raster (row blocks) */
  PinBuf<int> h_map;                /* staging (row blocks): the map on its way up, the finished table on its way down - a copy to */
  PinBuf<wdpm_pond> h_table;        /* or from pageable memory would make the host wait inside the queueing step */
  DevBuf<PondRow> table;
  int nb = 0;                       /* blocks of the scan */
  int rpw = 1;                      /* of the call under way */
  Status last = {};                 /* status words of the call under way */
  bool valid = false;               /* the last label call succeeded */
  PhaseTimer<WDPM_PONDS_PHASES + 2, WDPM_PONDS_PHASES> timer;   /* the host reads the status between scan and table: two marks there */
  wdpm_pond_stats stats = {};
};
struct RimUnit {                    /* wdpm_pond_rims.hip: the table of the last wdpm_rims_label; every label call takes `valid` away first */
  DevBuf<RimRow> table;
  bool valid = false;
  PhaseTimer<WDPM_RIMS_PHASES + 1, WDPM_RIMS_PHASES> timer;
  /* a row block (wdpm_group_rims_label): the table then holds one row per SLOT - the rank's local ponds, then its foreign ponds -
   * and slot_of[label in the whole raster] says which */
  DevBuf<int> slot_of;
  DevBuf<int> foreign;              /* 2 x g.ncp: the foreign ponds' labels */
  PinBuf<unsigned long long> h_beside;   /* staging: 2 x g.nsc wet masks, 2 x g.ncp labels of the rows beside the rank's own, 2 x g.ncp foreign labels */
  PinBuf<wdpm_pond_rim> h_table;    /* the finished rim rows on their way down */
  long long slots = 0, nforeign = 0;   /* of the call under way */
  std::vector<int> slot_label;      /* slot -> label in the whole raster */
};
struct CatchUnit {                  /* wdpm_pond_catchments.hip: likewise for wdpm_catch_label */
  DevBuf<int> link;                 /* g.rows x g.ncp: the link raster, the basin raster once a call has ended */
  DevBuf<CatchRow> table;
  StatusPair<CatchStatus> status;
  bool valid = false;
  /* events: init | receivers | jump rounds | tally, finish; row blocks: 0-1 receivers, 2-3 a batch of jump rounds, 4-5 tally */
  PhaseTimer<kCatchEvents, WDPM_CATCH_PHASES> timer;
  wdpm_pond_catchment_stats stats = {};
  /* a row block (wdpm_group_catch_label): the table then holds one row per SLOT - the rims' slots, then the rank's remote ponds -
   * and the link raster's rows 0 and g.rows - 1 belong to the neighbours */
  DevBuf<unsigned long long> keys;  /* 4 x g.ncp level keys: the rank's first and last owned row, then the rows beside them */
  PinBuf<unsigned long long> h_keys;   /* laid out likewise: two rows on their way down, two on their way up */
  DevBuf<int> exits;                /* 4 x g.ncp: where each exit ends (2 x g.ncp), the remote ponds' labels */
  PinBuf<int> h_exits;              /* 6 x g.ncp: the links of the first and last owned row on their way down (and, behind the tally, the */
                                    /* same rows as basins: the seam basins of the outlet pass), then as `exits` */
  PinBuf<wdpm_pond_catchment> h_table;   /* the finished catchment rows on their way down */
  long long slots = 0, remote = 0;  /* of the call under way */
  int rounds = 0;
  std::vector<int> remote_label;    /* the whole-raster labels of the remote slots, which follow the rims' slots (slot_label) */
};
struct OutletUnit {                 /* wdpm_pond_outlets.hip: likewise for wdpm_outlets_label */
  DevBuf<OutletRow> table;
  StatusPair<OutletStatus> status;
  bool valid = false;
  PhaseTimer<WDPM_OUTLETS_PHASES + 1, WDPM_OUTLETS_PHASES> timer;   /* init, passes | locate, finish */
  wdpm_pond_outlet_stats stats = {};
  /* a row block (wdpm_group_outlets_label): the table then holds one row per SLOT, as the catchments' does.  keys and h_keys grow
   * together, for C slots at a time */
  DevBuf<unsigned long long> keys;  /* 2 x C: every slot's pour key and divide count on their way down, the merged keys on their way up */
  PinBuf<unsigned long long> h_keys;   /* 3 x C: keys and counts as they came down, then, behind the 2 x slots words of the call, the merged keys */
  PinBuf<OutletRow> h_table;        /* the slots' rows on their way down */
  PinBuf<int> h_seam;               /* 2 x g.ncp: the facing ranks' seam basins on their way up */
};
struct CurveUnit {                  /* wdpm_pond_curves.hip: likewise for wdpm_curves_label */
  DevBuf<CurveRow> table;
  StatusPair<CurveStatus> status;
  bool valid = false;
  PhaseTimer<WDPM_CURVES_PHASES + 1, WDPM_CURVES_PHASES> timer;     /* init, bed | stages, finish */
  wdpm_pond_curve_stats stats = {};
  /* a row block (wdpm_group_curves_label): the table then holds one row per SLOT, as the outlets' does */
  DevBuf<unsigned long long> keys;  /* C: every slot's bed key on its way down, the merged keys on their way up */
  PinBuf<unsigned long long> h_keys;   /* 2 x C: the keys as they came down, then, behind the slots words of the call, the merged keys */
  PinBuf<CurveRow> h_table;         /* the slots' rows on their way down */
};

struct SpillUnit {                  /* wdpm_pond_spills.hip: likewise for wdpm_spill_label; whole rasters only */
  DevBuf<wdpm_pond_spill> table;
  DevBuf<int> words;                /* 15 x N: next, flags, ring marks, and the pointers and hop counts of the passes, two buffers each */
  DevBuf<unsigned long long> sums;  /* 14 x N: per-pond values, path sums (two buffers), the five subtree sums (two buffers) */
  StatusPair<SpillStatus> status;
  bool valid = false;
  PhaseTimer<WDPM_SPILL_PHASES + 1, WDPM_SPILL_PHASES> timer;       /* init, ring rounds, cut | chain rounds | sum rounds, finish */
  wdpm_pond_spill_stats stats = {};
};

struct RouteUnit {                  /* wdpm_pond_routing.hip: likewise for wdpm_route_label and wdpm_route_rerun; whole rasters only */
  DevBuf<wdpm_pond_route> table;
  DevBuf<int> words;                /* 3 x N: next, level and the ponds in level order; then levels + 1 offsets and as many cursors */
  DevBuf<unsigned long long> sums;  /* 5 x N: area, fill_q, and what the feeders add: in_q, reach_ponds, reach_cells */
  StatusPair<RouteStatus> status;
  PinBuf<int> h_offsets;            /* the levels + 1 offsets on their way down, once per label call */
  bool valid = false;               /* the table, and with it everything a rerun stands on */
  int narrow = kBlock, run_levels = kRouteRunLevels;   /* WDPM_ROUTE_NARROW, WDPM_ROUTE_RUN_LEVELS when the handle was made */
  int levels = 0;                   /* of the last label call */
  RoutePlan plan;
  PhaseTimer<5, WDPM_ROUTE_PHASES> timer;                           /* order | (the host plans) | sweep | finish */
  wdpm_pond_route_stats stats = {};
};

/* a merged table of a group: what the last label call of its kind left; every label call takes `valid` away first */
template <class Row, class Stats> struct Merged {
  std::vector<Row> rows;
  bool valid = false;
  Stats stats = {};
};

}  // namespace wdpm_pond_detail
#pragma GCC visibility pop

/* The handle labels a VIEW of its context: rows [row_off, row_off + g.rows) of the context's rasters, whose first and last row the
 * kernels take for the dry border.  wdpm_ponds_create views a whole-raster context; a row block of a group (wdpm_group_ponds_*) is
 * viewed as its owned rows with one row either side.
 * A new buffer is one member of its unit's record, as a holder, and one line in release() (wdpm_ponds.hip): nothing else. */
struct wdpm_ponds {
  wdpm_ctx *x = nullptr;
  wdpm_pond_detail::Geom g = {};
  int row_off = 0;                  /* context row of the view's row 0 */
  bool seams = false;               /* a row block: the labels of rows 1 and g.rows - 2 come to the host with the status */
  size_t guard = 0;                 /* bytes of each guard band (WDPM_GUARD_KB when the handle was made) */
  std::vector<wdpm_pond_detail::Guarded> guards;
  int forced_rpw = 0;               /* WDPM_PONDS_ROWS_PER_WAVE when the handle was made, 0: the library chooses */
  bool timing = false;              /* WDPM_PONDS_TIMING=1 when the handle was made: HIP events around every kernel */
  wdpm_pond_detail::LabelUnit lab;
  wdpm_pond_detail::RimUnit rim;
  wdpm_pond_detail::CatchUnit cat;
  wdpm_pond_detail::OutletUnit out;
  wdpm_pond_detail::CurveUnit cur;
  wdpm_pond_detail::SpillUnit spl;
  wdpm_pond_detail::RouteUnit rte;
};

/* the handle of include/wdpm_group_ponds.h, include/wdpm_group_pond_rims.h, include/wdpm_group_pond_catchments.h,
 * include/wdpm_group_pond_outlets.h and include/wdpm_group_pond_curves.h */
struct wdpm_group_ponds {
  wdpm_group *grp = nullptr;
  int n = 0;                               /* ranks */
  int rows = 0, ncp = 0;                   /* the whole raster, padded */
  std::vector<wdpm_ponds *> r;             /* one handle per rank, on its owned rows with one row either side */
  std::vector<int> own_lo, own_rows, view0;   /* whole-raster rows: first owned, how many owned, the view's row 0 */
  bool timing = true;                      /* until a rank's handle records no events */
  wdpm_pond_detail::Merged<wdpm_pond, wdpm_group_pond_stats> lab;
  wdpm_pond_detail::Merged<wdpm_pond_rim, wdpm_group_rim_stats> rim;
  wdpm_pond_detail::Merged<wdpm_pond_catchment, wdpm_group_catchment_stats> cat;
  wdpm_pond_detail::Merged<wdpm_pond_outlet, wdpm_group_outlet_stats> out;
  wdpm_pond_detail::Merged<wdpm_pond_curve, wdpm_group_curve_stats> cur;
};

#pragma GCC visibility push(hidden)
namespace wdpm_pond_detail {
/* wdpm_group_ponds_label, and with `rims` what wdpm_group_rims_label adds to it: after rank i's table kernels are queued and
 * before any rank is waited for, rims(h, i, map) queues that rank's rim work, map[rank][local label - 1] being the stitch's
 * numbers.  One wait per rank then ends both. */
typedef int (*group_rims_queue)(wdpm_group_ponds *h, int rank, const std::vector<std::vector<int>> &map, long long ponds);
/* `seams` (may be null): called for rank i right after its scan is queued and before any rank is waited for, so that what it
 * sends to the host arrives with the seam labels. */
typedef int (*group_seams_queue)(wdpm_group_ponds *h, int rank);
int group_label(wdpm_group_ponds *h, double min_depth, int64_t *nponds, group_rims_queue rims, group_seams_queue seams = nullptr);
/* wdpm_pond_rims.hip: the rims argument of wdpm_group_rims_label, and what that call does once group_label has returned - the
 * ranks' rim rows merged into h->rim, h->lab.valid and h->rim.valid set.  wdpm_group_catch_label runs both and adds its own. */
int group_rims_rank(wdpm_group_ponds *h, int rank, const std::vector<std::vector<int>> &map, long long ponds);
int group_rims_merge(wdpm_group_ponds *h, const char *caller, long long ponds);
/* after a failure with work queued: let every rank's stream run dry, so that nothing still reads what the caller may free; the
 * message stays */
int group_drain(wdpm_group_ponds *h);

inline double ms_between(const timespec &a, const timespec &b) { return (double)(b.tv_sec - a.tv_sec) * 1e3 + (double)(b.tv_nsec - a.tv_nsec) * 1e-6; }

/* the owned rows [ra, rb) of rank i in rows of its view; halo: bit 0 a rank above, bit 1 a rank below */
struct OwnedRows { int ra, rb, halo; };
inline OwnedRows owned_rows(const wdpm_group_ponds *gh, int i) {
  const int ra = gh->own_lo[i] - gh->view0[i];
  return {ra, ra + gh->own_rows[i], (i > 0 ? 1 : 0) | (i + 1 < gh->n ? 2 : 0)};
}

/* the waves of a kernel that walks `rows` rows of the view down its segment columns, each wave rpw rows of one column */
struct Waves { int rpw, nwaves; };
inline Waves waves_for(const wdpm_ponds *h, int rows) {
  const int rpw = ponds_rows_per_wave(h->g.nseg, h->g.rows, h->forced_rpw);
  return {rpw, ((rows + rpw - 1) / rpw) * h->g.nsc};
}

/* ---- what every unit's entry points check and hand out, in the order the headers under include/ promise ---- */
inline int check_min_depth(const char *caller, double v) {
  return (!(v >= 0.0) || std::isinf(v)) ? wdpm_fail("%s: min_depth must be finite and >= 0 (got %g)", caller, v) : 0;
}
/* `joint`: the two oldest units (labels, rims) answer a null handle and a null output with one message */
inline int check_args(const char *caller, const void *h, const void *out, bool joint) {
  if (joint) return (!h || !out) ? wdpm_fail("%s: null argument", caller) : 0;
  if (!h) return wdpm_fail("%s: null handle", caller);
  return out ? 0 : wdpm_fail("%s: null output", caller);
}
/* `bytes` of the handle's device memory to the caller's pageable memory, behind everything the context has queued */
inline int download(wdpm_ponds *h, void *out, const void *dev, size_t bytes) {
  if (wdpm_synchronize(h->x)) return 1;
  HIP_TRY(hipMemcpyAsync(out, dev, bytes, hipMemcpyDeviceToHost, h->x->stream));
  return wdpm_stream_sync(h->x, h->x->stream);
}
template <class U> int copy_rows(wdpm_ponds *h, U &u, void *out, size_t bytes) { return download(h, out, u.table.p, bytes); }
template <class U> int copy_rows(wdpm_group_ponds *, U &u, void *out, size_t bytes) { memcpy(out, u.rows.data(), bytes); return 0; }

/* *_table of handle type H (whole raster or group) and unit `unit`; `none` is the sentence for a handle without that table */
template <class H, class U, class Row>
int table_out(const char *caller, H *h, U H::*unit, const char *none, Row *out, int64_t capacity) {
  if (!h) return wdpm_fail("%s: null handle", caller);
  if (!h->lab.valid || !(h->*unit).valid) return wdpm_fail("%s: %s", caller, none);
  const long long n = h->lab.stats.ponds;
  if (capacity < n) return wdpm_fail("%s: capacity %lld is too small for %lld ponds", caller, (long long)capacity, n);
  if (n == 0) return 0;
  if (!out) return wdpm_fail("%s: null output", caller);
  return copy_rows(h, h->*unit, out, (size_t)n * sizeof(Row));
}
template <class H, class U, class S>
int stats_out(const char *caller, H *h, U H::*unit, const char *none, S *out, bool joint = false) {
  if (check_args(caller, h, out, joint)) return 1;
  if (!h->lab.valid || !(h->*unit).valid) return wdpm_fail("%s: %s", caller, none);
  *out = (h->*unit).stats;
  return 0;
}
/* *_phase_ms: `valid` is the handle's own unit, or the group's while `h` is one of its ranks */
template <class U>
int phase_ms_tail(const char *caller, bool timing, bool valid, const char *none, const wdpm_ponds *h, U wdpm_ponds::*unit, double *ms) {
  if (!timing) return wdpm_fail("%s: the handle records no events (set WDPM_PONDS_TIMING=1 before it is made)", caller);
  if (!valid) return wdpm_fail("%s: %s", caller, none);
  for (int i = 0; i < (h->*unit).timer.phases; i++) ms[i] = (h->*unit).timer.ms[i];
  return 0;
}
template <class U>
int phase_ms_out(const char *caller, wdpm_ponds *h, U wdpm_ponds::*unit, const char *none, double *ms, bool joint = false) {
  if (check_args(caller, h, ms, joint)) return 1;
  return phase_ms_tail(caller, h->timing, h->lab.valid && (h->*unit).valid, none, h, unit, ms);
}
template <class G, class U>
int group_phase_ms_out(const char *caller, wdpm_group_ponds *h, G wdpm_group_ponds::*merged, U wdpm_ponds::*unit, const char *none, int32_t rank, double *ms,
                       bool joint = false) {
  if (check_args(caller, h, ms, joint)) return 1;
  if (rank < 0 || rank >= h->n) return wdpm_fail("%s: rank %d of %d", caller, rank, h->n);
  return phase_ms_tail(caller, h->timing, h->lab.valid && (h->*merged).valid, none, h->r[rank], unit, ms);
}
}  // namespace wdpm_pond_detail
#pragma GCC visibility pop
#endif

#endif
