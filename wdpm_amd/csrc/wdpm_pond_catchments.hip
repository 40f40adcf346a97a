/*
 * wdpm_pond_catchments.hip — the catchment of every pond (include/wdpm_pond_catchments.h): which pond every dry cell drains to,
 * from the label raster, the wet masks, the DEM and the water a label call leaves on the device.  gfx950.  A unit of its own
 * beside wdpm_ponds.hip and wdpm_pond_rims.hip: not in the launch ledger, not among the sources wdpm_build_info() hashes.
 *
 *   receivers  Shaped like the rim kernel: a wave owns one 64-column segment over rows_per_wave rows (ponds_rows_per_wave) and
 *              keeps a sliding three-row window of level keys and labels in registers; column neighbours come from the lanes
 *              next door, those of lanes 0 and 63 from memory.  One int32 LINK per cell: the view-local padded index of the
 *              receiver when that is a slope cell itself, else a terminal code - pond k as -1 - k (a pond cell, or a slope cell
 *              whose receiver is one: the label is in the window), a pit as -1, a cell without a level as INT_MIN.  Chains so
 *              run over slope cells only.  A row whose lanes are all pond cells or border (the wet masks say so) reads neither
 *              dem nor w.  Slope cells and pits are counted per wave; inflow cells per wave BY LABEL, carried down the rows
 *   jump       pointer jumping, one thread per cell, in rounds the host queues in small batches: a cell whose link is no
 *              terminal follows kCatchHops links, or up to a terminal, and stores what it reached.  Links are read and written
 *              as relaxed agent-scope atomics; every value a cell ever holds is a later cell of its own descent or the descent's
 *              terminal, so a stale read costs time and nothing else.  A thread counts itself unresolved from the value IT
 *              stores; the count goes out once per wave and reaches the host through pinned memory.  A round at least halves
 *              every descent.  A round that finds the round before it left nothing returns at once
 *   tally      the table kernel's scheme over the links, which are all terminals now: per wave BY LABEL - ballots of the slope
 *              lanes that hold basin k, a popcount, a butterfly maximum over the level keys, ctz / clz for the columns - carried
 *              down the rows while the label stays, one set of atomics per (wave, label change), extremes after a look.  It
 *              rewrites the link raster in place into basin(c).  init takes each pond's box from its pond-table row, finish turns
 *              the head key into a double
 *
 * tests/catch_emu_main.cpp compiles the kernels for the host under sanitizers with WDPM_PONDS_EMULATION defined, as
 * tests/rims_emu_main.cpp does with wdpm_pond_rims.hip, and leaves the host half out.
 */
#include "wdpm_ponds_priv.h"

using namespace wdpm_pond_detail;

namespace {

constexpr unsigned long long kNoLevel = ~0ull;     /* no level's key: the image of a NaN no addition makes */
constexpr int kLinkPit = -1;                       /* pond k is -1 - k */
constexpr int kLinkNone = INT_MIN;

__device__ __forceinline__ int load_link(const int *p, int i) {
  return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* the key of a level: dem + w where there is water to add, dem where there is none (NaN, zero, negative); none without dem < +inf */
__device__ __forceinline__ unsigned long long level_key(double e, double d) {
  return e < __builtin_inf() ? depth_key(d > 0.0 ? e + d : e) : kNoLevel;
}

/* level key of the interior cell (r, c) */
__device__ __forceinline__ unsigned long long level_of(const double *__restrict__ w, const double *__restrict__ dem, const Geom &g, int r, int c) {
  const int idx = r * g.ncp + c;
  return level_key(dem[idx], w[idx]);
}

/* one row of the window.  m is wave-uniform.  ek and el belong to the cell beside the segment: lane 0 holds the one on the left,
 * lane 63 the one on the right. */
struct CatchWin {
  unsigned long long m, key, ek;
  int lbl, el;
  bool has;
};

__device__ __forceinline__ CatchWin catch_open(const unsigned long long *__restrict__ masks, const Geom &g, int r, int s) {
  CatchWin w;
  w.m = (r >= 0 && r < g.rows) ? masks[(long long)r * g.nsc + s] : 0ull;
  w.key = w.ek = kNoLevel;
  w.lbl = w.el = 0;
  w.has = false;
  return w;
}

/* Keys and labels of row r: a dry lane's label is 0 by its mask; border cells and cells beyond the raster have no level and are
 * not read.  Every load is issued before the first is used: dem and w of a cell do not wait for each other. */
__device__ __forceinline__ void catch_fill(CatchWin &x, const double *__restrict__ w, const double *__restrict__ dem,
                                           const int *__restrict__ labels, const Geom &g, int r, int c, int lane) {
  if (x.has) return;
  x.has = true;
  if (r < 1 || r > g.rows - 2) return;
  const int ce = lane == 0 ? c - 1 : c + 1;                  /* the cell beside the segment: lanes 0 and 63 */
  const bool own = c >= 1 && c <= g.ncp - 2, beside = (lane == 0 || lane == 63) && ce >= 1 && ce <= g.ncp - 2;
  const int idx = r * g.ncp + c, idxe = r * g.ncp + ce;
  double e = __builtin_inf(), d = 0.0, ee = __builtin_inf(), de = 0.0;
  if (own) {
    e = dem[idx];
    d = w[idx];
    if (bit(x.m, lane)) x.lbl = labels[idx];
  }
  if (beside) {
    ee = dem[idxe];
    de = w[idxe];
    x.el = labels[idxe];                                      /* 0 on whatever is no pond cell */
  }
  x.key = level_key(e, d);
  x.ek = level_key(ee, de);
}

/* ---- receivers ------------------------------------------------------------------------------------------------------------- */
/* Everything that steers the loops is wave-uniform. */
__global__ __launch_bounds__(kBlock) void catch_receivers_kernel(const double *__restrict__ w, const double *__restrict__ dem,
                                                                 const unsigned long long *__restrict__ masks,
                                                                 const int *__restrict__ labels, Geom g, int rpw, int nwaves,
                                                                 int *__restrict__ link, CatchRow *table, CatchStatus *st) {
  const int wid = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (wid >= nwaves) return;
  const int lane = threadIdx.x & 63;
  const int strip = wid / g.nsc, s = wid - strip * g.nsc;
  const int r0 = strip * rpw, r1 = min(r0 + rpw, g.rows);
  const int c = s * kSeg + lane;
  const bool inside = c < g.ncp;
  const unsigned long long edgem = __ballot(c < 1 || c > g.ncp - 2);     /* border columns and what lies beyond the raster */
  unsigned long long n_slope = 0ull, n_pit = 0ull, cy_n = 0ull;
  int cy_label = 0;                        /* inflow cells held for one label and not yet sent */

  CatchWin up = catch_open(masks, g, r0 - 1, s), cur = catch_open(masks, g, r0, s), dn;
  for (int r = r0; r < r1; r++, up = cur, cur = dn) {
    dn = catch_open(masks, g, r + 1, s);
    const int idx = r * g.ncp + c;
    const bool wet = bit(cur.m, lane);
    if (r < 1 || r > g.rows - 2 || (cur.m | edgem) == ~0ull) {            /* pond cells and border: the labels say it all */
      if (inside) link[idx] = wet ? -1 - labels[idx] : kLinkNone;
      continue;
    }
    catch_fill(up, w, dem, labels, g, r - 1, c, lane);
    catch_fill(cur, w, dem, labels, g, r, c, lane);
    catch_fill(dn, w, dem, labels, g, r + 1, c, lane);
    /* the eight neighbours in the order of their padded index */
    const unsigned long long nk[8] = {lane_from_left(up.key, up.ek, lane),   up.key, lane_from_right(up.key, up.ek, lane),
                                      lane_from_left(cur.key, cur.ek, lane),         lane_from_right(cur.key, cur.ek, lane),
                                      lane_from_left(dn.key, dn.ek, lane),   dn.key, lane_from_right(dn.key, dn.ek, lane)};
    const int nl[8] = {lane_from_left(up.lbl, up.el, lane),   up.lbl, lane_from_right(up.lbl, up.el, lane),
                       lane_from_left(cur.lbl, cur.el, lane),         lane_from_right(cur.lbl, cur.el, lane),
                       lane_from_left(dn.lbl, dn.el, lane),   dn.lbl, lane_from_right(dn.lbl, dn.el, lane)};
    const bool slope = inside && !wet && cur.key != kNoLevel;
    unsigned long long best = cur.key;     /* strictly below the cell's own, the first of equals */
    int to = 0, to_label = 0;
    bool found = false;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int dr = (i < 3 ? -1 : i < 5 ? 0 : 1), dc = (i < 3 ? i - 1 : i == 3 ? -1 : i == 4 ? 1 : i - 6);
      if (nk[i] < best) {
        best = nk[i];
        to = idx + dr * g.ncp + dc;
        to_label = nl[i];
        found = true;
      }
    }
    const bool pit = slope && !found;
    const int inflow = slope && found ? to_label : 0;      /* the pond this cell's water enters, 0: none */
    if (inside) link[idx] = wet ? -1 - cur.lbl : !slope ? kLinkNone : pit ? kLinkPit : inflow ? -1 - inflow : to;
    n_slope += (unsigned long long)__popcll(__ballot(slope));
    n_pit += (unsigned long long)__popcll(__ballot(pit));

    /* inflow cells per wave, by label */
    int cand = inflow;
    for (;;) {
      const unsigned long long pending = __ballot(cand != 0);
      if (pending == 0ull) break;
      const int L = __shfl(cand, __builtin_ctzll(pending));
      const unsigned long long hitm = __ballot(cand == L);
      if (cy_label != L) {                 /* down the rows: the same label goes on gathering, another one sends first */
        if (cy_label != 0 && lane == 0) atomicAdd(&table[cy_label - 1].inflow_cells, cy_n);
        cy_label = L;
        cy_n = 0ull;
      }
      cy_n += (unsigned long long)__popcll(hitm);
      if (cand == L) cand = 0;
    }
  }
  if (lane == 0) {
    if (cy_label != 0) atomicAdd(&table[cy_label - 1].inflow_cells, cy_n);
    if (n_slope) atomicAdd(&st->slope, n_slope);
    if (n_pit) atomicAdd(&st->pit, n_pit);
  }
}

/* ---- jump ------------------------------------------------------------------------------------------------------------------ */
__global__ __launch_bounds__(kBlock) void catch_jump_kernel(int *link, int ncells, int round, CatchStatus *st) {
  if (round > 0 && st->unres[round - 1] == 0u) return;       /* the round before left nothing (block-uniform) */
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  bool unresolved = false;
  if (i < ncells) {
    int v = load_link(link, (int)i);
    if (v >= 0) {
#pragma unroll 1
      for (int hop = 0; hop < kCatchHops && v >= 0; hop++) v = load_link(link, v);
      __hip_atomic_store(link + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      unresolved = v >= 0;
    }
  }
  const unsigned long long um = __ballot(unresolved);
  if (um != 0ull && (threadIdx.x & 63) == 0) atomicAdd(&st->unres[round], (unsigned)__popcll(um));
}

/* ---- tally ----------------------------------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(kBlock) void catch_init_kernel(CatchRow *t, const PondRow *__restrict__ ponds, long long n) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  CatchRow r;
  r.catch_cells = r.inflow_cells = r.head_key = 0ull;
  r.row_min = ponds[i].row_min;
  r.row_max = ponds[i].row_max;
  r.col_min = ponds[i].col_min;
  r.col_max = ponds[i].col_max;
  t[i] = r;
}

__global__ __launch_bounds__(kBlock) void catch_finish_kernel(CatchRow *t, long long n) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const double d = t[i].catch_cells ? depth_from_key(t[i].head_key) : -__builtin_inf();
  t[i].head_key = (unsigned long long)__double_as_longlong(d);
}

/* what a wave has gathered for one label and not yet sent */
struct CatchCarry {
  int label;               /* 0: nothing held */
  unsigned long long cells, key;
  int row_min, row_max, col_min, col_max;
};

/* one lane sends a carry: the extrema through atomic_min_if / atomic_max_if */
__device__ __forceinline__ void catch_send(CatchRow *table, const CatchCarry &c) {
  CatchRow *t = table + (c.label - 1);
  atomicAdd(&t->catch_cells, c.cells);
  atomic_max_if(&t->head_key, c.key);
  atomic_min_if(&t->row_min, c.row_min);
  atomic_max_if(&t->row_max, c.row_max);
  atomic_min_if(&t->col_min, c.col_min);
  atomic_max_if(&t->col_max, c.col_max);
}

__global__ __launch_bounds__(kBlock) void catch_tally_kernel(const double *__restrict__ w, const double *__restrict__ dem,
                                                             const unsigned long long *__restrict__ masks, Geom g, int rpw,
                                                             int nwaves, int *link, CatchRow *table, CatchStatus *st) {
  const int wid = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (wid >= nwaves) return;
  const int lane = threadIdx.x & 63;
  const int strip = wid / g.nsc, s = wid - strip * g.nsc;
  const int r0 = strip * rpw, r1 = min(r0 + rpw, g.rows);
  const int c = s * kSeg + lane;
  const bool inside = c < g.ncp;
  unsigned long long n_unponded = 0ull;
  CatchCarry cy;
  cy.label = 0; cy.cells = cy.key = 0ull;
  cy.row_min = cy.col_min = INT_MAX; cy.row_max = cy.col_max = -1;

  for (int r = r0; r < r1; r++) {
    const unsigned long long m = masks[(long long)r * g.nsc + s];
    const int idx = r * g.ncp + c;
    const int v = inside ? link[idx] : kLinkNone;
    const int basin = v == kLinkNone ? -1 : -1 - v;        /* a pit's -1 is 0, pond k's -1 - k is k */
    if (inside) link[idx] = basin;
    const bool slope = !bit(m, lane) && v != kLinkNone;
    n_unponded += (unsigned long long)__popcll(__ballot(slope && basin == 0));
    int cand = slope && basin > 0 ? basin : 0;
    if (__ballot(cand != 0) == 0ull) continue;
    unsigned long long key = 0ull;
    if (cand) key = level_of(w, dem, g, r, c);
    for (;;) {
      const unsigned long long pending = __ballot(cand != 0);
      if (pending == 0ull) break;
      const int L = __shfl(cand, __builtin_ctzll(pending));
      const unsigned long long hitm = __ballot(cand == L);
      const unsigned long long hi = wave_max(cand == L ? key : 0ull);
      const int cmin = s * kSeg + __builtin_ctzll(hitm), cmax = s * kSeg + 63 - __clzll((long long)hitm);
      if (cy.label != L) {                  /* down the rows: the same label goes on gathering, another one sends first */
        if (cy.label != 0 && lane == 0) catch_send(table, cy);
        cy.label = L; cy.cells = cy.key = 0ull;
        cy.row_min = r; cy.col_min = INT_MAX; cy.row_max = cy.col_max = -1;
      }
      cy.cells += (unsigned long long)__popcll(hitm);
      cy.key = hi > cy.key ? hi : cy.key;
      cy.row_max = r;
      cy.col_min = min(cy.col_min, cmin);
      cy.col_max = max(cy.col_max, cmax);
      if (cand == L) cand = 0;
    }
  }
  if (lane == 0) {
    if (cy.label != 0) catch_send(table, cy);
    if (n_unponded) atomicAdd(&st->unponded, n_unponded);
  }
}

}  // namespace

#ifndef WDPM_PONDS_EMULATION
/* ---- host ------------------------------------------------------------------------------------------------------------------ */
namespace {
const char kNoTable[] = "no catchment table: the last label call on this handle was not a wdpm_catch_label that succeeded";
}  // namespace

extern "C" int wdpm_catch_label(wdpm_ponds *h, double min_depth, int64_t *nponds) {
  if (!h) return wdpm_fail("wdpm_catch_label: null handle");
  if (!(min_depth >= 0.0) || std::isinf(min_depth)) return wdpm_fail("wdpm_catch_label: min_depth must be finite and >= 0 (got %g)", min_depth);
  if (h->seams) return wdpm_fail("wdpm_catch_label: the handle views a row block: catchments are taken on whole rasters only");
  const Geom g = h->g;
  const long long cells = (long long)g.rows * g.ncp;
  if (cells > (long long)INT_MAX)
    return wdpm_fail("wdpm_catch_label: the view holds %lld cells, more than 2^31 - 1: a link is an int32 cell index", cells);
  int64_t n = 0;
  if (wdpm_rims_label(h, min_depth, &n)) return 1;            /* leaves masks, labels, both tables and the stream as this pass wants them */
  wdpm_ctx *x = h->x;
  const hipStream_t sm = x->stream;
  HIP_TRY(hipSetDevice(x->p.device));
  if (!h->d_link) {
    const hipError_t e = guarded_malloc(h, (void **)&h->d_link, (size_t)cells * sizeof(int));
    if (e != hipSuccess) { h->d_link = nullptr; return wdpm_fail("wdpm_catch_label: no device memory for the links of %lld cells: %s", cells, hipGetErrorString(e)); }
  }
  if (!h->d_cstat) {
    hipError_t e = hipMalloc(&h->d_cstat, sizeof(CatchStatus));
    if (e != hipSuccess) { h->d_cstat = nullptr; return wdpm_fail("wdpm_catch_label: no device memory for the status words: %s", hipGetErrorString(e)); }
    e = hipHostMalloc(&h->h_cstat, sizeof(CatchStatus));
    if (e != hipSuccess) { h->h_cstat = nullptr; (void)hipFree(h->d_cstat); h->d_cstat = nullptr; return wdpm_fail("wdpm_catch_label: no pinned host memory for the status words: %s", hipGetErrorString(e)); }
  }
  if (n > h->catch_cap) {                                     /* sized from N, like the pond table */
    guarded_free(h, h->d_catch);
    h->d_catch = nullptr;
    h->catch_cap = 0;
    const hipError_t e = guarded_malloc(h, (void **)&h->d_catch, (size_t)n * sizeof(CatchRow));
    if (e != hipSuccess) return wdpm_fail("wdpm_catch_label: no device memory for the catchments of %lld ponds: %s", (long long)n, hipGetErrorString(e));
    h->catch_cap = n;
  }
  const size_t off = (size_t)h->row_off * g.ncp;
  const double *w = x->d_w[x->cur] + off, *dem = x->d_dem + off;
  const int rpw = ponds_rows_per_wave(g.nseg, g.rows, h->forced_rpw);
  const int nwaves = ((g.rows + rpw - 1) / rpw) * g.nsc;
  const unsigned nblocks = blocks_for(n, kBlock), wblocks = blocks_for(nwaves, kWaves), cblocks = blocks_for(cells, kBlock);
#define CATCH_MARK(i) do { if (h->timing) HIP_TRY(hipEventRecord(h->catch_ev[i], sm)); } while (0)
  HIP_TRY(hipMemsetAsync(h->d_cstat, 0, sizeof(CatchStatus), sm));
  CATCH_MARK(0);
  if (n > 0) hipLaunchKernelGGL(catch_init_kernel, dim3(nblocks), dim3(kBlock), 0, sm, h->d_catch, h->d_table, (long long)n);
  CATCH_MARK(1);
  hipLaunchKernelGGL(catch_receivers_kernel, dim3(wblocks), dim3(kBlock), 0, sm, w, dem, h->d_masks, h->d_labels, g, rpw, nwaves, h->d_link,
                     h->d_catch, h->d_cstat);
  CATCH_MARK(2);
  /* rounds in batches: one look of the host per batch.  A defect ends as an error here, never as a loop that goes on. */
  int rounds = 0;
  for (;;) {
    for (int b = 0; b < kCatchBatch; b++, rounds++)
      hipLaunchKernelGGL(catch_jump_kernel, dim3(cblocks), dim3(kBlock), 0, sm, h->d_link, (int)cells, rounds, h->d_cstat);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->h_cstat, h->d_cstat, sizeof(CatchStatus), hipMemcpyDeviceToHost, sm));
    if (wdpm_stream_sync(x, sm)) return 1;
    if (h->h_cstat->unres[rounds - 1] == 0u) break;
    if (rounds >= kCatchRoundCap)
      return wdpm_fail("wdpm_catch_label: %u cells are still on their way after %d rounds of pointer jumping, which halve every descent: "
                       "the link raster is damaged", h->h_cstat->unres[rounds - 1], rounds);
  }
  CATCH_MARK(3);
  hipLaunchKernelGGL(catch_tally_kernel, dim3(wblocks), dim3(kBlock), 0, sm, w, dem, h->d_masks, g, rpw, nwaves, h->d_link, h->d_catch,
                     h->d_cstat);
  if (n > 0) hipLaunchKernelGGL(catch_finish_kernel, dim3(nblocks), dim3(kBlock), 0, sm, h->d_catch, (long long)n);
  CATCH_MARK(4);
#undef CATCH_MARK
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h->h_cstat, h->d_cstat, sizeof(CatchStatus), hipMemcpyDeviceToHost, sm));
  if (wdpm_stream_sync(x, sm)) return 1;
  if (h->timing) {
    float ms[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < 4; i++) HIP_TRY(hipEventElapsedTime(&ms[i], h->catch_ev[i], h->catch_ev[i + 1]));
    h->catch_ms[0] = ms[1];
    h->catch_ms[1] = ms[2];
    h->catch_ms[2] = (double)ms[0] + (double)ms[3];
  }
  h->catch_stats.slope_cells = (int64_t)h->h_cstat->slope;
  h->catch_stats.pit_cells = (int64_t)h->h_cstat->pit;
  h->catch_stats.unponded_cells = (int64_t)h->h_cstat->unponded;
  h->catch_stats.rounds = rounds;
  h->catch_stats.ponds = n;
  h->catch_valid = true;
  if (nponds) *nponds = n;
  return 0;
}

extern "C" int wdpm_catch_table(wdpm_ponds *h, wdpm_pond_catchment *out, int64_t capacity) {
  if (!h) return wdpm_fail("wdpm_catch_table: null handle");
  if (!h->valid || !h->catch_valid) return wdpm_fail("wdpm_catch_table: %s", kNoTable);
  const long long n = h->stats.ponds;
  if (capacity < n) return wdpm_fail("wdpm_catch_table: capacity %lld is too small for %lld ponds", (long long)capacity, n);
  if (n == 0) return 0;
  if (!out) return wdpm_fail("wdpm_catch_table: null output");
  if (wdpm_synchronize(h->x)) return 1;
  HIP_TRY(hipMemcpyAsync(out, h->d_catch, (size_t)n * sizeof(wdpm_pond_catchment), hipMemcpyDeviceToHost, h->x->stream));
  return wdpm_stream_sync(h->x, h->x->stream);
}

extern "C" int wdpm_catch_basins(wdpm_ponds *h, int32_t *padded) {
  if (!h) return wdpm_fail("wdpm_catch_basins: null handle");
  if (!padded) return wdpm_fail("wdpm_catch_basins: null output");
  if (!h->valid || !h->catch_valid) return wdpm_fail("wdpm_catch_basins: %s", kNoTable);
  if (wdpm_synchronize(h->x)) return 1;
  HIP_TRY(hipMemcpyAsync(padded, h->d_link, (size_t)h->g.rows * h->g.ncp * sizeof(int32_t), hipMemcpyDeviceToHost, h->x->stream));
  return wdpm_stream_sync(h->x, h->x->stream);
}

extern "C" int wdpm_catch_stats(wdpm_ponds *h, wdpm_pond_catchment_stats *out) {
  if (!h) return wdpm_fail("wdpm_catch_stats: null handle");
  if (!out) return wdpm_fail("wdpm_catch_stats: null output");
  if (!h->valid || !h->catch_valid) return wdpm_fail("wdpm_catch_stats: %s", kNoTable);
  *out = h->catch_stats;
  return 0;
}

extern "C" int wdpm_catch_phase_ms(wdpm_ponds *h, double *ms) {
  if (!h) return wdpm_fail("wdpm_catch_phase_ms: null handle");
  if (!ms) return wdpm_fail("wdpm_catch_phase_ms: null output");
  if (!h->timing) return wdpm_fail("wdpm_catch_phase_ms: the handle records no events (set WDPM_PONDS_TIMING=1 before it is made)");
  if (!h->valid || !h->catch_valid) return wdpm_fail("wdpm_catch_phase_ms: %s", kNoTable);
  for (int i = 0; i < WDPM_CATCH_PHASES; i++) ms[i] = h->catch_ms[i];
  return 0;
}
#endif  /* WDPM_PONDS_EMULATION */
