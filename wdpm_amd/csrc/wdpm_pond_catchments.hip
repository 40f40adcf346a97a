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
 * Over row blocks (include/wdpm_group_pond_catchments.h) every rank runs the same bodies over its owned rows (kRows): the one row
 * beyond either end is known by its whole-raster labels (the rims' upload) and by the level keys its owner wrote
 * (catch_seam_keys_kernel), a receiver that is a slope cell of such a row makes the link an EXIT, the table is indexed through the
 * rims' label -> slot table, and the tally looks up where the host found each exit to end (wdpm_catch_stitch.h).
 *
 * tests/catch_emu_main.cpp and tests/group_catch_emu_main.cpp compile the kernels for the host under sanitizers with
 * WDPM_PONDS_EMULATION defined, as tests/rims_emu_main.cpp does with wdpm_pond_rims.hip, and leave the host half out.
 */
#include "wdpm_ponds_priv.h"

using namespace wdpm_pond_detail;

namespace {

constexpr unsigned long long kNoLevel = ~0ull;     /* no level's key: the image of a NaN no addition makes */
constexpr int kLinkPit = -1;                       /* pond k is -1 - k */
constexpr int kLinkNone = INT_MIN;
constexpr int kExitBase = INT_MIN + 1;             /* row blocks: the exit (side, column) is kExitBase + side * ncp + column */

/* What a row block's kernels know beyond a whole raster's (kRows; wave-uniform all of it): the owned rows [ra, rb) of the view,
 * over which the strips are cut; which of view rows 0 and g.rows - 1 belong to a neighbour (halo bit 0: the one above, bit 1: the
 * one below) - of those the labels and masks are the rims' upload, the level keys come from nkeys (2 x ncp, written by their
 * owners) and neither dem nor w is ever read; the table is indexed through slot_of; exit_basin (2 x ncp, the tally) says where
 * each exit ends. */
struct CatchRows {
  int ra, rb, halo;
  const unsigned long long *nkeys;
  const int *slot_of;
  const int *exit_basin;
};

template <bool kRows>
__device__ __forceinline__ int catch_slot(const CatchRows &rw, int L) {
  return kRows ? rw.slot_of[L] : L - 1;
}

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
template <bool kRows>
__device__ __forceinline__ void catch_fill(CatchWin &x, const double *__restrict__ w, const double *__restrict__ dem,
                                           const int *__restrict__ labels, const Geom &g, int r, int c, int lane, const CatchRows &rw) {
  if (x.has) return;
  x.has = true;
  const bool halo = kRows && ((r == 0 && (rw.halo & 1)) || (r == g.rows - 1 && (rw.halo & 2)));     /* a neighbour's row */
  if (!halo && (r < 1 || r > g.rows - 2)) return;
  const int ce = lane == 0 ? c - 1 : c + 1;                  /* the cell beside the segment: lanes 0 and 63 */
  const bool own = c >= 1 && c <= g.ncp - 2, beside = (lane == 0 || lane == 63) && ce >= 1 && ce <= g.ncp - 2;
  const int idx = r * g.ncp + c, idxe = r * g.ncp + ce;
  if (kRows && halo) {                                       /* its owner's keys; dem and w of a halo row are not current */
    const unsigned long long *nk = rw.nkeys + (r == 0 ? 0 : g.ncp);
    if (own) {
      x.key = nk[c];
      if (bit(x.m, lane)) x.lbl = labels[idx];
    }
    if (beside) {
      x.ek = nk[ce];
      x.el = labels[idxe];
    }
    return;
  }
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
template <bool kRows>
__device__ __forceinline__ void catch_receivers_body(const double *__restrict__ w, const double *__restrict__ dem,
                                                     const unsigned long long *__restrict__ masks, const int *__restrict__ labels,
                                                     const Geom &g, int rpw, int nwaves, int *__restrict__ link,
                                                     CatchRow *table, CatchStatus *st, const CatchRows &rw) {
  const int wid = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (wid >= nwaves) return;
  const int lane = threadIdx.x & 63;
  const int strip = wid / g.nsc, s = wid - strip * g.nsc;
  const int r0 = (kRows ? rw.ra : 0) + strip * rpw, r1 = min(r0 + rpw, kRows ? rw.rb : g.rows);
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
    catch_fill<kRows>(up, w, dem, labels, g, r - 1, c, lane, rw);
    catch_fill<kRows>(cur, w, dem, labels, g, r, c, lane, rw);
    catch_fill<kRows>(dn, w, dem, labels, g, r + 1, c, lane, rw);
    /* the eight neighbours in the order of their padded index */
    const unsigned long long nk[8] = {lane_from_left(up.key, up.ek, lane),   up.key, lane_from_right(up.key, up.ek, lane),
                                      lane_from_left(cur.key, cur.ek, lane),         lane_from_right(cur.key, cur.ek, lane),
                                      lane_from_left(dn.key, dn.ek, lane),   dn.key, lane_from_right(dn.key, dn.ek, lane)};
    const int nl[8] = {lane_from_left(up.lbl, up.el, lane),   up.lbl, lane_from_right(up.lbl, up.el, lane),
                       lane_from_left(cur.lbl, cur.el, lane),         lane_from_right(cur.lbl, cur.el, lane),
                       lane_from_left(dn.lbl, dn.el, lane),   dn.lbl, lane_from_right(dn.lbl, dn.el, lane)};
    const bool slope = inside && !wet && cur.key != kNoLevel;
    unsigned long long best = cur.key;     /* strictly below the cell's own, the first of equals */
    int to = 0, to_label = 0, to_dr = 0, to_dc = 0;
    bool found = false;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int dr = (i < 3 ? -1 : i < 5 ? 0 : 1), dc = (i < 3 ? i - 1 : i == 3 ? -1 : i == 4 ? 1 : i - 6);
      if (nk[i] < best) {
        best = nk[i];
        to = idx + dr * g.ncp + dc;
        to_label = nl[i];
        found = true;
        if (kRows) { to_dr = dr; to_dc = dc; }
      }
    }
    const bool pit = slope && !found;
    const int inflow = slope && found ? to_label : 0;      /* the pond this cell's water enters, 0: none */
    if (kRows) {                                           /* a receiver in a neighbour's row that is no pond cell: the descent exits */
      const bool up_out = r == 1 && (rw.halo & 1), dn_out = r == g.rows - 2 && (rw.halo & 2);
      if ((to_dr < 0 && up_out) || (to_dr > 0 && dn_out)) to = kExitBase + (to_dr > 0 ? g.ncp : 0) + c + to_dc;
    }
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
        if (cy_label != 0 && lane == 0) atomicAdd(&table[catch_slot<kRows>(rw, cy_label)].inflow_cells, cy_n);
        cy_label = L;
        cy_n = 0ull;
      }
      cy_n += (unsigned long long)__popcll(hitm);
      if (cand == L) cand = 0;
    }
  }
  if (lane == 0) {
    if (cy_label != 0) atomicAdd(&table[catch_slot<kRows>(rw, cy_label)].inflow_cells, cy_n);
    if (n_slope) atomicAdd(&st->slope, n_slope);
    if (n_pit) atomicAdd(&st->pit, n_pit);
  }
}

__global__ __launch_bounds__(kBlock) void catch_receivers_kernel(const double *__restrict__ w, const double *__restrict__ dem,
                                                                 const unsigned long long *__restrict__ masks,
                                                                 const int *__restrict__ labels, Geom g, int rpw, int nwaves,
                                                                 int *__restrict__ link, CatchRow *table, CatchStatus *st) {
  catch_receivers_body<false>(w, dem, masks, labels, g, rpw, nwaves, link, table, st, CatchRows());
}

/* the same over the owned rows of a row block's view */
__global__ __launch_bounds__(kBlock) void catch_receivers_rows_kernel(const double *__restrict__ w, const double *__restrict__ dem,
                                                                      const unsigned long long *__restrict__ masks,
                                                                      const int *__restrict__ labels, Geom g, int rpw, int nwaves,
                                                                      int *__restrict__ link, CatchRow *table, CatchStatus *st,
                                                                      CatchRows rw) {
  catch_receivers_body<true>(w, dem, masks, labels, g, rpw, nwaves, link, table, st, rw);
}

/* Row blocks, before the receivers: the level keys of the rank's first and last owned row (view rows 1 and g.rows - 2, as the seam
 * labels), 2 x ncp, for the neighbours - from the water that was labelled, which is on the device by now; and a terminal into the
 * links of the neighbours' rows, which no descent of this rank enters but every jump round looks at. */
__global__ __launch_bounds__(kBlock) void catch_seam_keys_kernel(const double *__restrict__ w, const double *__restrict__ dem, Geom g,
                                                                 int halo, unsigned long long *__restrict__ keys, int *__restrict__ link) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= 2 * g.ncp) return;
  const int side = i >= g.ncp, c = i - side * g.ncp, r = side ? g.rows - 2 : 1;
  keys[i] = c >= 1 && c <= g.ncp - 2 ? level_of(w, dem, g, r, c) : kNoLevel;
  if (halo & (1 << side)) link[(side ? g.rows - 1 : 0) * g.ncp + c] = kLinkNone;
}

/* row blocks: the table starts with empty boxes - the merge brings each pond's own */
__global__ __launch_bounds__(kBlock) void catch_init_rows_kernel(CatchRow *t, long long n) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  CatchRow r;
  r.catch_cells = r.inflow_cells = r.head_key = 0ull;
  r.row_min = r.col_min = INT_MAX;
  r.row_max = r.col_max = -1;
  t[i] = r;
}

/* row blocks, before the tally: remote pond j takes slot base + j (its entry of slot_of held no slot before) */
__global__ __launch_bounds__(kBlock) void catch_remote_slots_kernel(const int *__restrict__ remote, int nremote, int base, int *slot_of) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < nremote) slot_of[remote[i]] = base + i;
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
template <bool kRows>
__device__ __forceinline__ void catch_send(CatchRow *table, const CatchCarry &c, const CatchRows &rw) {
  CatchRow *t = table + catch_slot<kRows>(rw, c.label);
  atomicAdd(&t->catch_cells, c.cells);
  atomic_max_if(&t->head_key, c.key);
  atomic_min_if(&t->row_min, c.row_min);
  atomic_max_if(&t->row_max, c.row_max);
  atomic_min_if(&t->col_min, c.col_min);
  atomic_max_if(&t->col_max, c.col_max);
}

template <bool kRows>
__device__ __forceinline__ void catch_tally_body(const double *__restrict__ w, const double *__restrict__ dem,
                                                 const unsigned long long *__restrict__ masks, const Geom &g, int rpw,
                                                 int nwaves, int *link, CatchRow *table, CatchStatus *st, const CatchRows &rw) {
  const int wid = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (wid >= nwaves) return;
  const int lane = threadIdx.x & 63;
  const int strip = wid / g.nsc, s = wid - strip * g.nsc;
  const int r0 = (kRows ? rw.ra : 0) + strip * rpw, r1 = min(r0 + rpw, kRows ? rw.rb : g.rows);
  const int c = s * kSeg + lane;
  const bool inside = c < g.ncp;
  unsigned long long n_unponded = 0ull, n_exits = 0ull;
  CatchCarry cy;
  cy.label = 0; cy.cells = cy.key = 0ull;
  cy.row_min = cy.col_min = INT_MAX; cy.row_max = cy.col_max = -1;

  for (int r = r0; r < r1; r++) {
    const unsigned long long m = masks[(long long)r * g.nsc + s];
    const int idx = r * g.ncp + c;
    int v = inside ? link[idx] : kLinkNone;
    if (kRows) {                                           /* an exit: one look at where the host found it to end */
      const bool exits = v != kLinkNone && v <= kExitBase + (2 * g.ncp - 1);
      n_exits += (unsigned long long)__popcll(__ballot(exits));
      if (exits) v = rw.exit_basin[v - kExitBase];
    }
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
        if (cy.label != 0 && lane == 0) catch_send<kRows>(table, cy, rw);
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
    if (cy.label != 0) catch_send<kRows>(table, cy, rw);
    if (n_unponded) atomicAdd(&st->unponded, n_unponded);
    if (kRows && n_exits) atomicAdd(&st->exits, n_exits);
  }
}

__global__ __launch_bounds__(kBlock) void catch_tally_kernel(const double *__restrict__ w, const double *__restrict__ dem,
                                                             const unsigned long long *__restrict__ masks, Geom g, int rpw,
                                                             int nwaves, int *link, CatchRow *table, CatchStatus *st) {
  catch_tally_body<false>(w, dem, masks, g, rpw, nwaves, link, table, st, CatchRows());
}

/* the same over the owned rows of a row block's view; rows of the table's boxes stay rows of the view (the merge shifts them) */
__global__ __launch_bounds__(kBlock) void catch_tally_rows_kernel(const double *__restrict__ w, const double *__restrict__ dem,
                                                                  const unsigned long long *__restrict__ masks, Geom g, int rpw,
                                                                  int nwaves, int *link, CatchRow *table, CatchStatus *st,
                                                                  CatchRows rw) {
  catch_tally_body<true>(w, dem, masks, g, rpw, nwaves, link, table, st, rw);
}

}  // namespace

#ifndef WDPM_PONDS_EMULATION
/* ---- host ------------------------------------------------------------------------------------------------------------------ */
namespace {
const char kNoTable[] = "no catchment table: the last label call on this handle was not a wdpm_catch_label that succeeded";
}  // namespace

extern "C" int wdpm_catch_label(wdpm_ponds *h, double min_depth, int64_t *nponds) {
  if (!h) return wdpm_fail("wdpm_catch_label: null handle");
  if (check_min_depth("wdpm_catch_label", min_depth)) return 1;
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
  const char *what;
  hipError_t e = grow(h, h->cat.link, cells);
  if (e != hipSuccess) return wdpm_fail("wdpm_catch_label: no device memory for the links of %lld cells: %s", cells, hipGetErrorString(e));
  e = ensure(h->cat.status, &what);
  if (e != hipSuccess) return wdpm_fail("wdpm_catch_label: no %s memory for the status words: %s", what, hipGetErrorString(e));
  e = grow(h, h->cat.table, n);                               /* sized from N, like the pond table */
  if (e != hipSuccess) return wdpm_fail("wdpm_catch_label: no device memory for the catchments of %lld ponds: %s", (long long)n, hipGetErrorString(e));
  const size_t off = (size_t)h->row_off * g.ncp;
  const double *w = x->d_w[x->cur] + off, *dem = x->d_dem + off;
  const Waves wv = waves_for(h, g.rows);
  const int rpw = wv.rpw, nwaves = wv.nwaves;
  const unsigned nblocks = blocks_for(n, kBlock), wblocks = blocks_for(nwaves, kWaves), cblocks = blocks_for(cells, kBlock);
  HIP_TRY(hipMemsetAsync(h->cat.status.d, 0, sizeof(CatchStatus), sm));
  HIP_TRY(h->cat.timer.mark(h->timing, 0, sm));
  if (n > 0) hipLaunchKernelGGL(catch_init_kernel, dim3(nblocks), dim3(kBlock), 0, sm, h->cat.table.p, h->lab.table.p, (long long)n);
  HIP_TRY(h->cat.timer.mark(h->timing, 1, sm));
  hipLaunchKernelGGL(catch_receivers_kernel, dim3(wblocks), dim3(kBlock), 0, sm, w, dem, h->lab.masks.p, h->lab.labels.p, g, rpw, nwaves, h->cat.link.p,
                     h->cat.table.p, h->cat.status.d);
  HIP_TRY(h->cat.timer.mark(h->timing, 2, sm));
  /* rounds in batches: one look of the host per batch.  A defect ends as an error here, never as a loop that goes on. */
  int rounds = 0;
  for (;;) {
    for (int b = 0; b < kCatchBatch; b++, rounds++)
      hipLaunchKernelGGL(catch_jump_kernel, dim3(cblocks), dim3(kBlock), 0, sm, h->cat.link.p, (int)cells, rounds, h->cat.status.d);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->cat.status.h, h->cat.status.d, sizeof(CatchStatus), hipMemcpyDeviceToHost, sm));
    if (wdpm_stream_sync(x, sm)) return 1;
    if (h->cat.status.h->unres[rounds - 1] == 0u) break;
    if (rounds >= kCatchRoundCap)
      return wdpm_fail("wdpm_catch_label: %u cells are still on their way after %d rounds of pointer jumping, which halve every descent: "
                       "the link raster is damaged", h->cat.status.h->unres[rounds - 1], rounds);
  }
  HIP_TRY(h->cat.timer.mark(h->timing, 3, sm));
  hipLaunchKernelGGL(catch_tally_kernel, dim3(wblocks), dim3(kBlock), 0, sm, w, dem, h->lab.masks.p, g, rpw, nwaves, h->cat.link.p, h->cat.table.p,
                     h->cat.status.d);
  if (n > 0) hipLaunchKernelGGL(catch_finish_kernel, dim3(nblocks), dim3(kBlock), 0, sm, h->cat.table.p, (long long)n);
  HIP_TRY(h->cat.timer.mark(h->timing, 4, sm));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h->cat.status.h, h->cat.status.d, sizeof(CatchStatus), hipMemcpyDeviceToHost, sm));
  if (wdpm_stream_sync(x, sm)) return 1;
  if (h->timing) {
    double ms[4] = {0.0, 0.0, 0.0, 0.0};              /* init | receivers | jump rounds | tally, finish */
    for (int i = 0; i < 4; i++) HIP_TRY(h->cat.timer.read(i, i + 1, &ms[i]));
    h->cat.timer.ms[0] = ms[1];
    h->cat.timer.ms[1] = ms[2];
    h->cat.timer.ms[2] = ms[0] + ms[3];
  }
  h->cat.stats.slope_cells = (int64_t)h->cat.status.h->slope;
  h->cat.stats.pit_cells = (int64_t)h->cat.status.h->pit;
  h->cat.stats.unponded_cells = (int64_t)h->cat.status.h->unponded;
  h->cat.stats.rounds = rounds;
  h->cat.stats.ponds = n;
  h->cat.valid = true;
  if (nponds) *nponds = n;
  return 0;
}

extern "C" int wdpm_catch_table(wdpm_ponds *h, wdpm_pond_catchment *out, int64_t capacity) {
  return table_out("wdpm_catch_table", h, &wdpm_ponds::cat, kNoTable, out, capacity);
}

extern "C" int wdpm_catch_basins(wdpm_ponds *h, int32_t *padded) {
  if (check_args("wdpm_catch_basins", h, padded, false)) return 1;
  if (!h->lab.valid || !h->cat.valid) return wdpm_fail("wdpm_catch_basins: %s", kNoTable);
  return download(h, padded, h->cat.link.p, (size_t)h->g.rows * h->g.ncp * sizeof(int32_t));
}

extern "C" int wdpm_catch_stats(wdpm_ponds *h, wdpm_pond_catchment_stats *out) {
  return stats_out("wdpm_catch_stats", h, &wdpm_ponds::cat, kNoTable, out);
}

extern "C" int wdpm_catch_phase_ms(wdpm_ponds *h, double *ms) {
  return phase_ms_out("wdpm_catch_phase_ms", h, &wdpm_ponds::cat, kNoTable, ms);
}

/* ---- row blocks (include/wdpm_group_pond_catchments.h) ----------------------------------------------------------------------- */
#include "wdpm_catch_stitch.h"

namespace {
const char kNoGroupTable[] = "no catchment table: the last label call on this handle was not a wdpm_group_catch_label that succeeded";

CatchRows rows_of(const wdpm_group_ponds *gh, int i) {
  const wdpm_ponds *h = gh->r[i];
  const OwnedRows own = owned_rows(gh, i);
  return {own.ra, own.rb, own.halo, h->cat.keys.p + (size_t)2 * h->g.ncp, h->rim.slot_of.p, h->cat.exits.p};
}

/* Rank i's seam keys behind its scan (group_label calls this for every rank before the first wait): they reach the host with the
 * seam labels.  The rank's buffers are made here, at its first call. */
int group_catch_seams(wdpm_group_ponds *gh, int i) {
  wdpm_ponds *h = gh->r[i];
  wdpm_ctx *x = h->x;
  const Geom g = h->g;
  const hipStream_t sm = x->stream;
  const size_t ncp = (size_t)g.ncp;
  const long long cells = (long long)g.rows * g.ncp;
  HIP_TRY(hipSetDevice(x->p.device));
  const char *what;
  hipError_t e = grow(h, h->cat.link, cells);
  if (e != hipSuccess) return wdpm_fail("wdpm_group_catch_label: no device memory for the links of %lld cells: %s", cells, hipGetErrorString(e));
  e = ensure(h->cat.status, &what);
  if (e != hipSuccess) return wdpm_fail("wdpm_group_catch_label: no %s memory for the status words: %s", what, hipGetErrorString(e));
  e = grow(h, h->cat.keys, 4LL * g.ncp);
  if (e != hipSuccess) return wdpm_fail("wdpm_group_catch_label: no device memory for four rows of level keys: %s", hipGetErrorString(e));
  e = grow(h, h->cat.exits, 4LL * g.ncp);
  if (e != hipSuccess) return wdpm_fail("wdpm_group_catch_label: no device memory for four rows of exits: %s", hipGetErrorString(e));
  e = grow(h, h->cat.h_keys, 4LL * g.ncp);
  if (e != hipSuccess) return wdpm_fail("wdpm_group_catch_label: no pinned host memory for four rows of level keys: %s", hipGetErrorString(e));
  e = grow(h, h->cat.h_exits, 6LL * g.ncp);
  if (e != hipSuccess) return wdpm_fail("wdpm_group_catch_label: no pinned host memory for six rows of links: %s", hipGetErrorString(e));
  const size_t off = (size_t)h->row_off * ncp;
  const CatchRows rw = rows_of(gh, i);
  hipLaunchKernelGGL(catch_seam_keys_kernel, dim3(blocks_for(2 * g.ncp, kBlock)), dim3(kBlock), 0, sm, x->d_w[x->cur] + off, x->d_dem + off,
                     g, rw.halo, h->cat.keys.p, h->cat.link.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h->cat.h_keys.p, h->cat.keys.p, 2 * ncp * sizeof(unsigned long long), hipMemcpyDeviceToHost, sm));
  return 0;
}

/* one batch of jump rounds of rank i with the look that follows it on its way: the counts, and the links of the rank's first and
 * last owned row, which are final once the counts say so */
int group_catch_batch(wdpm_ponds *h) {
  const Geom g = h->g;
  const hipStream_t sm = h->x->stream;
  const long long cells = (long long)g.rows * g.ncp;
  HIP_TRY(h->cat.timer.mark(h->timing, 2, sm));
  for (int b = 0; b < kCatchBatch; b++, h->cat.rounds++)
    hipLaunchKernelGGL(catch_jump_kernel, dim3(blocks_for(cells, kBlock)), dim3(kBlock), 0, sm, h->cat.link.p, (int)cells, h->cat.rounds, h->cat.status.d);
  HIP_TRY(h->cat.timer.mark(h->timing, 3, sm));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h->cat.status.h, h->cat.status.d, sizeof(CatchStatus), hipMemcpyDeviceToHost, sm));
  HIP_TRY(hipMemcpyAsync(h->cat.h_exits.p, h->cat.link.p + (size_t)g.ncp, (size_t)g.ncp * sizeof(int), hipMemcpyDeviceToHost, sm));
  HIP_TRY(hipMemcpyAsync(h->cat.h_exits.p + g.ncp, h->cat.link.p + (size_t)(g.rows - 2) * g.ncp, (size_t)g.ncp * sizeof(int), hipMemcpyDeviceToHost, sm));
  return 0;
}

/* Rank i's rim work, then its receivers and its first batch of jump rounds, behind its table kernels, nothing waited for. */
int group_catch_rank(wdpm_group_ponds *gh, int i, const std::vector<std::vector<int>> &map, long long ponds) {
  if (group_rims_rank(gh, i, map, ponds)) return 1;
  wdpm_ponds *h = gh->r[i];
  wdpm_ctx *x = h->x;
  const Geom g = h->g;
  const hipStream_t sm = x->stream;
  const size_t ncp = (size_t)g.ncp;
  if (!wdpm_catch_stitch::codes_fit(ponds, g.ncp))
    return wdpm_fail("wdpm_group_catch_label: %lld ponds on %d padded columns: pond codes and exit codes of a link would meet "
                     "(N + 2 * columns + 2 > 2^31)", ponds, g.ncp);
  HIP_TRY(hipSetDevice(x->p.device));
  const long long held = h->rim.slots, cap = held + 2 * (long long)g.ncp;      /* the rims' slots, then up to 2 * ncp remote ponds */
  hipError_t e = grow(h, h->cat.table, cap);
  if (e != hipSuccess) return wdpm_fail("wdpm_group_catch_label: no device memory for %lld catchment rows: %s", cap, hipGetErrorString(e));
  e = grow(h, h->cat.h_table, cap);
  if (e != hipSuccess) return wdpm_fail("wdpm_group_catch_label: no pinned host memory for %lld catchment rows: %s", cap, hipGetErrorString(e));
  if (ponds > 0 && held == 0) {        /* the rim work made no slots: none of the whole raster's ponds lies in or beside these rows */
    e = grow(h, h->rim.slot_of, ponds + 1);
    if (e != hipSuccess) return wdpm_fail("wdpm_group_catch_label: no device memory for the slots of %lld ponds: %s", ponds, hipGetErrorString(e));
    HIP_TRY(hipMemsetAsync(h->rim.slot_of.p, 0x7f, (size_t)(ponds + 1) * sizeof(int), sm));
  }
  const CatchRows rw = rows_of(gh, i);
  for (int side = 0; side < 2; side++) {          /* the keys of the rows beside the rank's own, as their owners wrote them */
    if (!(rw.halo & (1 << side))) continue;
    const unsigned long long *src = gh->r[side ? i + 1 : i - 1]->cat.h_keys.p + (side ? 0 : ncp);
    unsigned long long *stage = h->cat.h_keys.p + (2 + side) * ncp;
    memcpy(stage, src, ncp * sizeof(unsigned long long));
    HIP_TRY(hipMemcpyAsync(h->cat.keys.p + (2 + side) * ncp, stage, ncp * sizeof(unsigned long long), hipMemcpyHostToDevice, sm));
  }
  const size_t off = (size_t)h->row_off * ncp;
  const double *w = x->d_w[x->cur] + off, *dem = x->d_dem + off;
  const Waves wv = waves_for(h, rw.rb - rw.ra);
  const int rpw = wv.rpw, nwaves = wv.nwaves;
  HIP_TRY(hipMemsetAsync(h->cat.status.d, 0, sizeof(CatchStatus), sm));
  HIP_TRY(h->cat.timer.mark(h->timing, 0, sm));
  hipLaunchKernelGGL(catch_init_rows_kernel, dim3(blocks_for(cap, kBlock)), dim3(kBlock), 0, sm, h->cat.table.p, cap);
  hipLaunchKernelGGL(catch_receivers_rows_kernel, dim3(blocks_for(nwaves, kWaves)), dim3(kBlock), 0, sm, w, dem, h->lab.masks.p, h->lab.labels.p, g,
                     rpw, nwaves, h->cat.link.p, h->cat.table.p, h->cat.status.d, rw);
  HIP_TRY(h->cat.timer.mark(h->timing, 1, sm));
  h->cat.rounds = 0;
  h->cat.slots = h->cat.remote = 0;
  h->cat.timer.clear();
  return group_catch_batch(h);
}

/* after a wait: the time of events a and b of rank p onto phase k */
int group_catch_time(wdpm_ponds *p, int a, int b, int k) {
  if (!p->timing) return 0;
  double ms = 0.0;
  HIP_TRY(p->cat.timer.read(a, b, &ms));
  p->cat.timer.ms[k] += ms;
  return 0;
}

}  // namespace

extern "C" int wdpm_group_catch_label(wdpm_group_ponds *h, double min_depth, int64_t *nponds) {
  if (!h) return wdpm_fail("wdpm_group_catch_label: null handle");
  if (check_min_depth("wdpm_group_catch_label", min_depth)) return 1;
  int64_t n = 0;
  /* every rank: scan, seam keys | stitch | table, rims, receivers, a first batch of jump rounds - and one wait per rank */
  if (group_label(h, min_depth, &n, group_catch_rank, group_catch_seams)) return 1;
  if (group_rims_merge(h, "wdpm_group_catch_label", n)) return 1;
  const int nr = h->n, ncp = h->ncp;
  for (int i = 0; i < nr; i++) {
    HIP_TRY(hipSetDevice(h->r[i]->x->p.device));
    if (group_catch_time(h->r[i], 0, 1, 0) || group_catch_time(h->r[i], 2, 3, 1)) return 1;
  }
  /* further batches for the ranks that need them: every rank's batch is queued before any rank's look */
  std::vector<char> open((size_t)nr);
  for (;;) {
    bool any = false;
    for (int i = 0; i < nr; i++) {
      wdpm_ponds *p = h->r[i];
      open[(size_t)i] = p->cat.status.h->unres[p->cat.rounds - 1] != 0u;
      if (!open[(size_t)i]) continue;
      any = true;
      if (p->cat.rounds >= kCatchRoundCap)
        return wdpm_fail("wdpm_group_catch_label: %u cells of rank %d are still on their way after %d rounds of pointer jumping, which "
                         "halve every descent: the link raster is damaged", p->cat.status.h->unres[p->cat.rounds - 1], i, p->cat.rounds);
    }
    if (!any) break;
    for (int i = 0; i < nr; i++)
      if (open[(size_t)i] && (hipSetDevice(h->r[i]->x->p.device) != hipSuccess || group_catch_batch(h->r[i]))) return group_drain(h);
    bool bad = false;
    std::string first_msg;
    for (int i = 0; i < nr; i++) {
      if (!open[(size_t)i]) continue;
      wdpm_ponds *p = h->r[i];
      if (hipSetDevice(p->x->p.device) != hipSuccess || wdpm_stream_sync(p->x, p->x->stream) || group_catch_time(p, 2, 3, 1)) {
        if (!bad) first_msg = wdpm_last_error();
        bad = true;
      }
    }
    if (bad) return wdpm_fail("%s", first_msg.c_str());
  }

  /* the exits: every rank's two rows of links are on the host */
  timespec t0, t1, t2, t3;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  std::vector<wdpm_catch_stitch::RankLinks> links((size_t)nr);
  for (int i = 0; i < nr; i++) {
    const wdpm_ponds *p = h->r[i];
    links[(size_t)i].top = p->cat.h_exits.p;
    links[(size_t)i].bottom = p->g.rows == 3 ? p->cat.h_exits.p : p->cat.h_exits.p + ncp;      /* one row between the view's first and last */
  }
  wdpm_catch_stitch::Resolved res;
  std::string err;
  if (wdpm_catch_stitch::resolve(links, ncp, res, err)) return wdpm_fail("wdpm_group_catch_label: %s", err.c_str());
  for (int i = 0; i < nr; i++) {
    wdpm_ponds *p = h->r[i];
    std::vector<int> &remote = p->cat.remote_label;
    wdpm_catch_stitch::remote_labels(res.exit_basin[(size_t)i], ncp, h->lab.rows.data(), h->view0[i], h->view0[i] + p->g.rows - 1, remote);
    p->cat.slots = (long long)(p->rim.slot_label.size() + remote.size());
    p->cat.remote = (long long)remote.size();
    if (p->cat.slots > p->cat.table.cap) return wdpm_fail("wdpm_group_catch_label: rank %d would hold %lld catchment rows of %lld", i, p->cat.slots, p->cat.table.cap);
    memcpy(p->cat.h_exits.p + (size_t)2 * ncp, res.exit_basin[(size_t)i].data(), (size_t)2 * ncp * sizeof(int));
    if (!remote.empty()) memcpy(p->cat.h_exits.p + (size_t)4 * ncp, remote.data(), remote.size() * sizeof(int));
  }
  clock_gettime(CLOCK_MONOTONIC, &t1);

  /* every rank: where its exits end, the slots of its remote ponds, tally and finish, its rows on their way down */
  for (int i = 0; i < nr; i++) {
    wdpm_ponds *p = h->r[i];
    wdpm_ctx *x = p->x;
    const Geom g = p->g;
    const hipStream_t sm = x->stream;
    const CatchRows rw = rows_of(h, i);
    const size_t off = (size_t)p->row_off * g.ncp;
    const double *w = x->d_w[x->cur] + off, *dem = x->d_dem + off;
    const Waves wv = waves_for(p, rw.rb - rw.ra);
    const int rpw = wv.rpw, nwaves = wv.nwaves;
    const int base = (int)(p->cat.slots - p->cat.remote);
    /* the first call that fails is the one the message names; nothing is queued behind it */
    hipError_t e = hipSetDevice(x->p.device);
    if (e == hipSuccess)
      e = hipMemcpyAsync(p->cat.exits.p, p->cat.h_exits.p + (size_t)2 * ncp, (size_t)(2 * ncp + p->cat.remote) * sizeof(int), hipMemcpyHostToDevice, sm);
    if (e == hipSuccess) e = p->cat.timer.mark(p->timing, 4, sm);
    if (e == hipSuccess) {
      if (p->cat.remote)
        hipLaunchKernelGGL(catch_remote_slots_kernel, dim3(blocks_for(p->cat.remote, kBlock)), dim3(kBlock), 0, sm, p->cat.exits.p + (size_t)2 * ncp,
                           (int)p->cat.remote, base, p->rim.slot_of.p);
      hipLaunchKernelGGL(catch_tally_rows_kernel, dim3(blocks_for(nwaves, kWaves)), dim3(kBlock), 0, sm, w, dem, p->lab.masks.p, g, rpw, nwaves,
                         p->cat.link.p, p->cat.table.p, p->cat.status.d, rw);
      if (p->cat.slots) hipLaunchKernelGGL(catch_finish_kernel, dim3(blocks_for(p->cat.slots, kBlock)), dim3(kBlock), 0, sm, p->cat.table.p, p->cat.slots);
      e = hipGetLastError();                                 /* of the launches */
    }
    if (e == hipSuccess) e = p->cat.timer.mark(p->timing, 5, sm);
    if (e == hipSuccess && p->cat.slots)
      e = hipMemcpyAsync(p->cat.h_table.p, p->cat.table.p, (size_t)p->cat.slots * sizeof(wdpm_pond_catchment), hipMemcpyDeviceToHost, sm);
    if (e == hipSuccess) e = hipMemcpyAsync(p->cat.status.h, p->cat.status.d, sizeof(CatchStatus), hipMemcpyDeviceToHost, sm);
    /* the rank's first and last owned row as basins, where their links lay: what an outlet pass hands the facing ranks */
    if (e == hipSuccess) e = hipMemcpyAsync(p->cat.h_exits.p, p->cat.link.p + (size_t)rw.ra * g.ncp, (size_t)g.ncp * sizeof(int), hipMemcpyDeviceToHost, sm);
    if (e == hipSuccess) e = hipMemcpyAsync(p->cat.h_exits.p + g.ncp, p->cat.link.p + (size_t)(rw.rb - 1) * g.ncp, (size_t)g.ncp * sizeof(int), hipMemcpyDeviceToHost, sm);
    if (e != hipSuccess) {
      (void)wdpm_fail("wdpm_group_catch_label: queueing the tally of rank %d failed: %s", i, hipGetErrorString(e));
      return group_drain(h);
    }
  }
  {
    bool bad = false;
    std::string first_msg;
    for (int i = 0; i < nr; i++) {
      wdpm_ponds *p = h->r[i];
      if (hipSetDevice(p->x->p.device) != hipSuccess || wdpm_stream_sync(p->x, p->x->stream) || group_catch_time(p, 4, 5, 2)) {
        if (!bad) first_msg = wdpm_last_error();
        bad = true;
      }
    }
    if (bad) return wdpm_fail("%s", first_msg.c_str());
  }

  clock_gettime(CLOCK_MONOTONIC, &t2);
  std::vector<wdpm_catch_stitch::RankCatch> ranks((size_t)nr);
  long long remote_sum = 0;
  for (int i = 0; i < nr; i++) {
    const wdpm_ponds *p = h->r[i];
    const CatchStatus &st = *p->cat.status.h;
    /* a remote slot was made for every pond a cell of the facing rows ends in; those that took a cell of this rank count */
    for (long long s = p->cat.slots - p->cat.remote; s < p->cat.slots; s++) remote_sum += p->cat.h_table.p[s].catch_cells > 0;
    ranks[(size_t)i] = {p->cat.h_table.p, p->rim.slot_label.data(), p->cat.slots, p->cat.remote_label.data(), p->cat.remote, h->view0[i], (long long)st.slope, (long long)st.pit,
                        (long long)st.unponded, (long long)st.exits, (long long)p->cat.rounds};
  }
  h->cat.rows.resize((size_t)n);
  wdpm_catch_stitch::Totals tot;
  if (wdpm_catch_stitch::merge(ranks, n, h->lab.rows.data(), h->cat.rows.data(), tot, err)) return wdpm_fail("wdpm_group_catch_label: %s", err.c_str());
  clock_gettime(CLOCK_MONOTONIC, &t3);
  h->cat.stats.slope_cells = tot.slope;
  h->cat.stats.pit_cells = tot.pit;
  h->cat.stats.unponded_cells = tot.unponded;
  h->cat.stats.rounds = tot.rounds;
  h->cat.stats.ponds = n;
  h->cat.stats.ranks = nr;
  h->cat.stats.exits = tot.exits;
  h->cat.stats.crossings = res.crossings;
  h->cat.stats.remote = remote_sum;
  h->cat.stats.resolve_ms = ms_between(t0, t1) + ms_between(t2, t3);
  h->cat.valid = true;
  if (nponds) *nponds = n;
  return 0;
}

extern "C" int wdpm_group_catch_table(wdpm_group_ponds *h, wdpm_pond_catchment *out, int64_t capacity) {
  return table_out("wdpm_group_catch_table", h, &wdpm_group_ponds::cat, kNoGroupTable, out, capacity);
}

extern "C" int wdpm_group_catch_basins(wdpm_group_ponds *h, int32_t *padded) {
  if (check_args("wdpm_group_catch_basins", h, padded, false)) return 1;
  if (!h->lab.valid || !h->cat.valid) return wdpm_fail("wdpm_group_catch_basins: %s", kNoGroupTable);
  /* every rank's owned rows, to where they lie in the whole raster, one after another as wdpm_group_ponds_labels brings them */
  for (int i = 0; i < h->n; i++) {
    wdpm_ponds *p = h->r[i];
    if (download(p, padded + (size_t)h->own_lo[i] * h->ncp, p->cat.link.p + (size_t)(h->own_lo[i] - h->view0[i]) * h->ncp,
                 (size_t)h->own_rows[i] * h->ncp * sizeof(int32_t)))
      return 1;
  }
  return 0;
}

extern "C" int wdpm_group_catch_stats(wdpm_group_ponds *h, wdpm_group_catchment_stats *out) {
  return stats_out("wdpm_group_catch_stats", h, &wdpm_group_ponds::cat, kNoGroupTable, out);
}

extern "C" int wdpm_group_catch_phase_ms(wdpm_group_ponds *h, int32_t rank, double *ms) {
  return group_phase_ms_out("wdpm_group_catch_phase_ms", h, &wdpm_group_ponds::cat, &wdpm_ponds::cat, kNoGroupTable, rank, ms);
}
#endif  /* WDPM_PONDS_EMULATION */
