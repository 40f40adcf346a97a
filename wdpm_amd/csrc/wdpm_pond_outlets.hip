/*
 * wdpm_pond_outlets.hip — the outlet of every pond (include/wdpm_pond_outlets.h): the lowest pass between a pond's basin and any
 * other, the cells on the divide, and what the basin floods and holds until it spills there; from the basin raster, the DEM and the
 * water a wdpm_catch_label leaves on the device.  gfx950.  A unit of its own beside wdpm_ponds.hip, wdpm_pond_rims.hip and
 * wdpm_pond_catchments.hip: not in the launch ledger, not among the sources wdpm_build_info() hashes.
 *
 * Shaped like the rim pair: a wave owns one 64-column segment over rows_per_wave rows (ponds_rows_per_wave) and keeps a sliding
 * three-row window in registers - the basins first, the level keys only when a row wants them; column neighbours come from the
 * lanes next door, those of lanes 0 and 63 from memory.
 *
 *   passes   A lane of basin k > 0 takes the minimum over its eight neighbours of max(own key, neighbour's key), over neighbours
 *            whose basin is >= 0 and another.  Then per wave BY LABEL: a ballot of the lanes that hold a pass of basin L, a popcount
 *            for the divide, a butterfly minimum; carried down the rows while the label stays, and one atomic_min_if on the pour
 *            key and one add of the divide count per (wave, label change).  A row whose own lanes hold no basin > 0, or whose three
 *            window rows - the cells beside the segment included - hold one basin >= 0 and no other, holds no pass and reads
 *            neither dem nor w: the settled all-wet raster, the inside of every large catchment
 *   locate   the same window, after every pour key is final (read once per (wave, label change)): a lane whose own minimum equals
 *            its pond's pour key offers from_index * 8 + direction to a 64-bit atomic_min_if, which is the tie rule.  In the same
 *            pass the lanes of basin L whose key lies below the pour key are counted and their rint((pour - level) * 2^24) summed
 *            by label, carried like the tally.  A row without a pass whose one pond has no outlet at all is skipped as above; a
 *            term of 512 m or more, or one that is not finite, sets a status word
 *   finish   index and direction to the four coordinates, to_basin from the basin raster, the key back to a double; +inf, -1 and
 *            zeros for a pond without a pass; the counts for wdpm_outlets_stats
 *
 * Over row blocks (include/wdpm_group_pond_outlets.h) every rank runs the same bodies over its owned rows (kRows) and owns every
 * pass (a, b) whose a lies there.  The one row beyond either end holds the whole-raster basins its owner sent (they go up into the
 * link raster's rows 0 and rows - 1) and is known by the level keys the catchment pass left in the rank's seam-key buffer: a halo
 * row's dem and w are never read.  The table is indexed through the label -> slot table of the rims and catchments.  The pour key
 * must be final over ALL ranks before anything is filled, so the host stands between passes and locate (wdpm_outlets_merge.h): the
 * ranks' keys come down, the lowest per pond goes back up, and locate offers view_index * 8 + direction against that key.
 *
 * Everything that steers a loop is wave-uniform.  tests/outlets_emu_main.cpp and tests/group_outlets_emu_main.cpp compile the
 * kernels for the host under sanitizers with WDPM_PONDS_EMULATION defined, as tests/catch_emu_main.cpp does with
 * wdpm_pond_catchments.hip, and leave the host half out.
 */
#include "wdpm_ponds_priv.h"

using namespace wdpm_pond_detail;

namespace {

constexpr unsigned long long kNone = ~0ull;        /* no pour key, no pair yet */

/* What a row block's kernels know beyond a whole raster's (kRows; wave-uniform all of it): the owned rows [ra, rb) of the view, over
 * which the strips are cut; which of view rows 0 and g.rows - 1 belong to a neighbour (halo bit 0: the one above, bit 1: the one
 * below) - of those the basins are their owner's, sent up into the link raster, the level keys come from nkeys (2 x ncp, written by
 * their owners) and neither dem nor w is ever read; the table is indexed through slot_of. */
struct OutRows {
  int ra, rb, halo;
  const unsigned long long *nkeys;
  const int *slot_of;
};

template <bool kRows>
__device__ __forceinline__ int out_slot(const OutRows &rw, int L) {
  return kRows ? rw.slot_of[L] : L - 1;
}

/* the key of the level of a cell that has one (basin >= 0): dem + w where there is water to add, dem where there is none */
__device__ __forceinline__ unsigned long long level_key(double e, double d) { return depth_key(d > 0.0 ? e + d : e); }

/* butterfly: every lane ends with the wave's sum */
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

/* One row of the window.  eb and ek belong to the cell beside the segment: lane 0 holds the one on the left, lane 63 the one on
 * the right, every other lane -1.  val, mixed and pond are wave-uniform. */
struct OutWin {
  int b, eb;
  unsigned long long key, ek;
  int val;                 /* a basin >= 0 of the row or beside it, -1: there is none */
  bool mixed;              /* ... and another one */
  bool pond;               /* a lane of the segment holds a basin > 0 */
  bool has;                /* the keys are filled */
};

/* The basins of row r (-1 outside the raster) and what the wave-uniform tests want of them; nothing of the levels yet.  Both loads
 * are issued before either is used. */
__device__ __forceinline__ OutWin out_open(const int *__restrict__ basins, const Geom &g, int r, int c, int lane) {
  OutWin x;
  x.b = x.eb = -1;
  x.key = x.ek = 0ull;
  x.has = false;
  if (r >= 0 && r < g.rows) {
    const int ce = lane == 0 ? c - 1 : c + 1;
    const bool own = c < g.ncp, beside = (lane == 0 || lane == 63) && ce >= 0 && ce < g.ncp;
    if (own) x.b = basins[r * g.ncp + c];
    if (beside) x.eb = basins[r * g.ncp + ce];
  }
  const unsigned long long in = __ballot(x.b >= 0), ein = __ballot(x.eb >= 0);
  x.val = in ? __shfl(x.b, __builtin_ctzll(in)) : ein ? __shfl(x.eb, __builtin_ctzll(ein)) : -1;
  x.mixed = __ballot((x.b >= 0 && x.b != x.val) || (x.eb >= 0 && x.eb != x.val)) != 0ull;
  x.pond = __ballot(x.b > 0) != 0ull;
  return x;
}

/* no pass starts in the row `cur` */
__device__ __forceinline__ bool out_quiet(const OutWin &up, const OutWin &cur, const OutWin &dn) {
  if (!cur.pond) return true;
  if (up.mixed || cur.mixed || dn.mixed) return false;
  return (up.val < 0 || up.val == cur.val) && (dn.val < 0 || dn.val == cur.val);
}

/* Level keys of row r's cells that have a basin (those alone have a level and lie inside the raster).  Every load is issued before
 * the first is used: dem and w of a cell do not wait for each other.  A neighbour's row (kRows) brings its owner's keys. */
template <bool kRows>
__device__ __forceinline__ void out_fill(OutWin &x, const double *__restrict__ w, const double *__restrict__ dem, const Geom &g, int r,
                                         int c, int lane, const OutRows &rw) {
  if (x.has) return;
  x.has = true;
  if (x.val < 0) return;
  const int ce = lane == 0 ? c - 1 : c + 1;
  if (kRows && ((r == 0 && (rw.halo & 1)) || (r == g.rows - 1 && (rw.halo & 2)))) {     /* dem and w of a halo row are not current */
    const unsigned long long *nk = rw.nkeys + (r == 0 ? 0 : g.ncp);
    if (x.b >= 0) x.key = nk[c];
    if (x.eb >= 0) x.ek = nk[ce];
    return;
  }
  double e = 0.0, d = 0.0, ee = 0.0, de = 0.0;
  if (x.b >= 0) {
    e = dem[r * g.ncp + c];
    d = w[r * g.ncp + c];
  }
  if (x.eb >= 0) {
    ee = dem[r * g.ncp + ce];
    de = w[r * g.ncp + ce];
  }
  x.key = level_key(e, d);
  x.ek = level_key(ee, de);
}

/* This lane's lowest pass: over the eight neighbours in the order of their padded index, those of another basin >= 0; the first of
 * equals stays.  Every lane takes part in the exchanges. */
__device__ __forceinline__ bool out_lowest(const OutWin &up, const OutWin &cur, const OutWin &dn, int lane, unsigned long long &height,
                                           int &dir) {
  const unsigned long long nk[8] = {lane_from_left(up.key, up.ek, lane),   up.key, lane_from_right(up.key, up.ek, lane),
                                    lane_from_left(cur.key, cur.ek, lane),         lane_from_right(cur.key, cur.ek, lane),
                                    lane_from_left(dn.key, dn.ek, lane),   dn.key, lane_from_right(dn.key, dn.ek, lane)};
  const int nb[8] = {lane_from_left(up.b, up.eb, lane),   up.b, lane_from_right(up.b, up.eb, lane),
                     lane_from_left(cur.b, cur.eb, lane),       lane_from_right(cur.b, cur.eb, lane),
                     lane_from_left(dn.b, dn.eb, lane),   dn.b, lane_from_right(dn.b, dn.eb, lane)};
  bool found = false;
  height = kNone;
  dir = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const unsigned long long hi = nk[i] > cur.key ? nk[i] : cur.key;
    if (cur.b > 0 && nb[i] >= 0 && nb[i] != cur.b && (!found || hi < height)) {
      height = hi;
      dir = i;
      found = true;
    }
  }
  return found;
}

/* ---- passes ---------------------------------------------------------------------------------------------------------------- */
template <bool kRows>
__device__ __forceinline__ void outlet_passes_body(const double *__restrict__ w, const double *__restrict__ dem,
                                                   const int *__restrict__ basins, const Geom &g, int rpw, int nwaves, OutletRow *table,
                                                   const OutRows &rw) {
  const int wid = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (wid >= nwaves) return;
  const int lane = threadIdx.x & 63;
  const int strip = wid / g.nsc, s = wid - strip * g.nsc;
  const int r0 = (kRows ? rw.ra : 0) + strip * rpw, r1 = min(r0 + rpw, kRows ? rw.rb : g.rows);
  const int c = s * kSeg + lane;
  int cy_label = 0;                        /* what the wave holds for one label and has not yet sent */
  unsigned long long cy_min = kNone, cy_divide = 0ull;

  OutWin up = out_open(basins, g, r0 - 1, c, lane), cur = out_open(basins, g, r0, c, lane), dn;
  for (int r = r0; r < r1; r++, up = cur, cur = dn) {
    dn = out_open(basins, g, r + 1, c, lane);
    if (out_quiet(up, cur, dn)) continue;
    out_fill<kRows>(up, w, dem, g, r - 1, c, lane, rw);
    out_fill<kRows>(cur, w, dem, g, r, c, lane, rw);
    out_fill<kRows>(dn, w, dem, g, r + 1, c, lane, rw);
    unsigned long long height;
    int dir;
    const bool found = out_lowest(up, cur, dn, lane, height, dir);

    /* per wave, by label */
    int cand = found ? cur.b : 0;
    for (;;) {
      const unsigned long long pending = __ballot(cand != 0);
      if (pending == 0ull) break;
      const int L = __shfl(cand, __builtin_ctzll(pending));
      const unsigned long long hitm = __ballot(cand == L);
      const unsigned long long lo = wave_min(cand == L ? height : kNone);
      if (cy_label != L) {                 /* down the rows: the same label goes on gathering, another one sends first */
        if (cy_label != 0 && lane == 0) {
          OutletRow *t = table + out_slot<kRows>(rw, cy_label);
          atomic_min_if(&t->pour_key, cy_min);
          atomicAdd(&t->divide_cells, cy_divide);
        }
        cy_label = L;
        cy_min = kNone;
        cy_divide = 0ull;
      }
      cy_min = lo < cy_min ? lo : cy_min;
      cy_divide += (unsigned long long)__popcll(hitm);
      if (cand == L) cand = 0;
    }
  }
  if (cy_label != 0 && lane == 0) {
    OutletRow *t = table + out_slot<kRows>(rw, cy_label);
    atomic_min_if(&t->pour_key, cy_min);
    atomicAdd(&t->divide_cells, cy_divide);
  }
}

__global__ __launch_bounds__(kBlock) void outlet_passes_kernel(const double *__restrict__ w, const double *__restrict__ dem,
                                                               const int *__restrict__ basins, Geom g, int rpw, int nwaves,
                                                               OutletRow *table) {
  outlet_passes_body<false>(w, dem, basins, g, rpw, nwaves, table, OutRows());
}

/* the same over the owned rows of a row block's view: every pass (a, b) whose a the rank owns */
__global__ __launch_bounds__(kBlock) void outlet_passes_rows_kernel(const double *__restrict__ w, const double *__restrict__ dem,
                                                                    const int *__restrict__ basins, Geom g, int rpw, int nwaves,
                                                                    OutletRow *table, OutRows rw) {
  outlet_passes_body<true>(w, dem, basins, g, rpw, nwaves, table, rw);
}

/* ---- locate ---------------------------------------------------------------------------------------------------------------- */
/* what a wave of the locate pass holds for one label */
struct FillCarry {
  int label;               /* 0: nothing held */
  int slot;                /* the label's table row */
  unsigned long long pour, cells, q;
};

/* the carry turns to label L: what it held goes out, and L's final pour key comes in.  A whole raster's row is L - 1 and needs no
 * slot: the carry's stays unused there. */
template <bool kRows>
__device__ __forceinline__ void fill_turn(FillCarry &cy, OutletRow *table, int L, int lane, const OutRows &rw) {
  if (cy.label == L) return;
  if (cy.label != 0 && cy.cells != 0ull && lane == 0) {
    atomicAdd(&table[kRows ? cy.slot : cy.label - 1].fill_cells, cy.cells);
    atomicAdd(&table[kRows ? cy.slot : cy.label - 1].fill_q, cy.q);
  }
  cy.label = L;
  if (kRows) cy.slot = L ? rw.slot_of[L] : 0;
  cy.pour = L ? table[kRows ? cy.slot : L - 1].pour_key : kNone;
  cy.cells = cy.q = 0ull;
}

template <bool kRows>
__device__ __forceinline__ void outlet_locate_body(const double *__restrict__ w, const double *__restrict__ dem,
                                                   const int *__restrict__ basins, const Geom &g, int rpw, int nwaves, OutletRow *table,
                                                   OutletStatus *st, const OutRows &rw) {
  const int wid = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (wid >= nwaves) return;
  const int lane = threadIdx.x & 63;
  const int strip = wid / g.nsc, s = wid - strip * g.nsc;
  const int r0 = (kRows ? rw.ra : 0) + strip * rpw, r1 = min(r0 + rpw, kRows ? rw.rb : g.rows);
  const int c = s * kSeg + lane;
  FillCarry cy;
  cy.label = 0;
  cy.slot = 0;
  cy.pour = kNone;
  cy.cells = cy.q = 0ull;

  OutWin up = out_open(basins, g, r0 - 1, c, lane), cur = out_open(basins, g, r0, c, lane), dn;
  for (int r = r0; r < r1; r++, up = cur, cur = dn) {
    dn = out_open(basins, g, r + 1, c, lane);
    if (!cur.pond) continue;
    const bool quiet = out_quiet(up, cur, dn);
    if (quiet) {                           /* one basin, cur.val > 0, and no pass here: without an outlet there is nothing to fill */
      fill_turn<kRows>(cy, table, cur.val, lane, rw);
      if (cy.pour == kNone) continue;
    }
    out_fill<kRows>(cur, w, dem, g, r, c, lane, rw);
    unsigned long long height = kNone;
    int dir = 0;
    bool found = false;
    if (!quiet) {
      out_fill<kRows>(up, w, dem, g, r - 1, c, lane, rw);
      out_fill<kRows>(dn, w, dem, g, r + 1, c, lane, rw);
      found = out_lowest(up, cur, dn, lane, height, dir);
    }

    int cand = cur.b > 0 ? cur.b : 0;
    for (;;) {
      const unsigned long long pending = __ballot(cand != 0);
      if (pending == 0ull) break;
      const int L = __shfl(cand, __builtin_ctzll(pending));
      fill_turn<kRows>(cy, table, L, lane, rw);
      const bool mine = cand == L;
      if (mine && found && height == cy.pour)
        atomic_min_if(&table[kRows ? cy.slot : L - 1].pair, (unsigned long long)(r * g.ncp + c) * 8ull + (unsigned long long)dir);
      const bool below = mine && cy.pour != kNone && cur.key < cy.pour;
      const unsigned long long belowm = __ballot(below);
      if (belowm != 0ull) {
        const double depth = depth_from_key(cy.pour) - depth_from_key(cur.key);
        const bool bad = below && !(depth < 512.0);          /* 512 m or more, +inf, NaN */
        if (bad) st->deep = 1u;
        cy.cells += (unsigned long long)__popcll(__ballot(below && !bad));
        cy.q += wave_sum(below && !bad ? (unsigned long long)rint(depth * 16777216.0) : 0ull);
      }
      if (mine) cand = 0;
    }
  }
  fill_turn<kRows>(cy, table, 0, lane, rw);
}

__global__ __launch_bounds__(kBlock) void outlet_locate_kernel(const double *__restrict__ w, const double *__restrict__ dem,
                                                               const int *__restrict__ basins, Geom g, int rpw, int nwaves,
                                                               OutletRow *table, OutletStatus *st) {
  outlet_locate_body<false>(w, dem, basins, g, rpw, nwaves, table, st, OutRows());
}

/* the same over the owned rows of a row block's view, against the pour keys the host merged over all ranks: the pair is a view
 * index, and a rank that holds fill cells of a pond and none of its passes fills to the right level all the same */
__global__ __launch_bounds__(kBlock) void outlet_locate_rows_kernel(const double *__restrict__ w, const double *__restrict__ dem,
                                                                    const int *__restrict__ basins, Geom g, int rpw, int nwaves,
                                                                    OutletRow *table, OutletStatus *st, OutRows rw) {
  outlet_locate_body<true>(w, dem, basins, g, rpw, nwaves, table, st, rw);
}

/* ---- init, finish ---------------------------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(kBlock) void outlet_init_kernel(OutletRow *t, long long n) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  OutletRow r;
  r.pour_key = r.pair = kNone;
  r.spare = 0ull;
  r.to_basin = -1;
  r.reserved = 0;
  r.divide_cells = r.fill_cells = r.fill_q = 0ull;
  t[i] = r;
}

/* two int32 as they lie in memory, the first at the lower address */
__device__ __forceinline__ unsigned long long two_ints(int first, int second) {
  return (unsigned long long)(unsigned)first | ((unsigned long long)(unsigned)second << 32);
}

/* the accumulated row becomes a wdpm_pond_outlet in place; every lane stays for the counts */
__global__ __launch_bounds__(kBlock) void outlet_finish_kernel(OutletRow *t, long long n, const int *__restrict__ basins, int ncp,
                                                               OutletStatus *st) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < n;
  bool none = false, land = false;
  unsigned long long divide = 0ull;
  if (live) {
    OutletRow r = t[i];
    none = r.pair == kNone || r.pour_key == kNone;
    if (none) {
      r.pour_key = (unsigned long long)__double_as_longlong(__builtin_inf());
      r.pair = r.spare = two_ints(-1, -1);
      r.to_basin = -1;
      r.divide_cells = r.fill_cells = r.fill_q = 0ull;
    } else {
      const int from = (int)(r.pair >> 3), i8 = (int)(r.pair & 7ull);
      const int dr = (i8 < 3 ? -1 : i8 < 5 ? 0 : 1), dc = (i8 < 3 ? i8 - 1 : i8 == 3 ? -1 : i8 == 4 ? 1 : i8 - 6);
      const int row = from / ncp, col = from - row * ncp;
      r.pour_key = (unsigned long long)__double_as_longlong(depth_from_key(r.pour_key));
      r.pair = two_ints(row, col);
      r.spare = two_ints(row + dr, col + dc);
      r.to_basin = basins[from + dr * ncp + dc];
      land = r.to_basin == 0;
      divide = r.divide_cells;
    }
    r.reserved = 0;
    t[i] = r;
  }
  const unsigned long long nonem = __ballot(none), landm = __ballot(land);
  divide = wave_sum(divide);
  if ((threadIdx.x & 63) == 0) {
    if (nonem) atomicAdd(&st->no_outlet, (unsigned long long)__popcll(nonem));
    if (landm) atomicAdd(&st->to_land, (unsigned long long)__popcll(landm));
    if (divide) atomicAdd(&st->divide, divide);
  }
}

/* ---- row blocks: what goes between the ranks and the host -------------------------------------------------------------------- */
/* after the passes: every slot's pour key and divide count, side by side for one copy down (n keys, then n counts) */
__global__ __launch_bounds__(kBlock) void outlet_pour_down_kernel(const OutletRow *__restrict__ t, long long n, unsigned long long *__restrict__ out) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  out[i] = t[i].pour_key;
  out[n + i] = t[i].divide_cells;
}

/* before the locate pass: every slot takes its pond's pour key as the host merged it over all ranks */
__global__ __launch_bounds__(kBlock) void outlet_pour_up_kernel(OutletRow *__restrict__ t, long long n, const unsigned long long *__restrict__ keys) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) t[i].pour_key = keys[i];
}

/* after the locate pass: to_basin of every slot that offered a pair, from the view - the pair's b may lie in a neighbour's row, whose
 * basins the view holds.  Key and pair stay as they are: the host decodes the winner's (wdpm_outlets_merge.h). */
__global__ __launch_bounds__(kBlock) void outlet_finish_rows_kernel(OutletRow *t, long long n, const int *__restrict__ basins, int ncp) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const unsigned long long pair = t[i].pair;
  if (pair == kNone) return;
  const int from = (int)(pair >> 3), i8 = (int)(pair & 7ull);
  const int dr = (i8 < 3 ? -1 : i8 < 5 ? 0 : 1), dc = (i8 < 3 ? i8 - 1 : i8 == 3 ? -1 : i8 == 4 ? 1 : i8 - 6);
  t[i].to_basin = basins[from + dr * ncp + dc];
}

}  // namespace

#ifndef WDPM_PONDS_EMULATION
/* ---- host ------------------------------------------------------------------------------------------------------------------ */
namespace {
const char kNoTable[] = "no outlet table: the last label call on this handle was not a wdpm_outlets_label that succeeded";
}  // namespace

extern "C" int wdpm_outlets_label(wdpm_ponds *h, double min_depth, int64_t *nponds) {
  if (!h) return wdpm_fail("wdpm_outlets_label: null handle");
  if (check_min_depth("wdpm_outlets_label", min_depth)) return 1;
  if (h->seams) return wdpm_fail("wdpm_outlets_label: the handle views a row block: outlets are taken on whole rasters only");
  int64_t n = 0;
  if (wdpm_catch_label(h, min_depth, &n)) return 1;           /* leaves the basin raster and the stream as this pass wants them */
  h->lab.valid = false;                                       /* a wdpm_outlets_label that fails leaves no table of any kind */
  wdpm_ctx *x = h->x;
  const Geom g = h->g;
  const hipStream_t sm = x->stream;
  HIP_TRY(hipSetDevice(x->p.device));
  const char *what;
  hipError_t e = ensure(h->out.status, &what);
  if (e != hipSuccess) return wdpm_fail("wdpm_outlets_label: no %s memory for the status words: %s", what, hipGetErrorString(e));
  e = grow(h, h->out.table, n);                               /* sized from N, like the pond table */
  if (e != hipSuccess) return wdpm_fail("wdpm_outlets_label: no device memory for the outlets of %lld ponds: %s", (long long)n, hipGetErrorString(e));
  h->out.timer.clear();
  memset(h->out.status.h, 0, sizeof(OutletStatus));
  if (n > 0) {                                                /* no pond, no outlet: nothing to launch */
    const size_t off = (size_t)h->row_off * g.ncp;
    const double *w = x->d_w[x->cur] + off, *dem = x->d_dem + off;
    const Waves wv = waves_for(h, g.rows);
    const int rpw = wv.rpw, nwaves = wv.nwaves;
    const unsigned nblocks = blocks_for(n, kBlock), wblocks = blocks_for(nwaves, kWaves);
    HIP_TRY(hipMemsetAsync(h->out.status.d, 0, sizeof(OutletStatus), sm));
    HIP_TRY(h->out.timer.mark(h->timing, 0, sm));
    hipLaunchKernelGGL(outlet_init_kernel, dim3(nblocks), dim3(kBlock), 0, sm, h->out.table.p, (long long)n);
    hipLaunchKernelGGL(outlet_passes_kernel, dim3(wblocks), dim3(kBlock), 0, sm, w, dem, h->cat.link.p, g, rpw, nwaves, h->out.table.p);
    HIP_TRY(h->out.timer.mark(h->timing, 1, sm));
    hipLaunchKernelGGL(outlet_locate_kernel, dim3(wblocks), dim3(kBlock), 0, sm, w, dem, h->cat.link.p, g, rpw, nwaves, h->out.table.p, h->out.status.d);
    hipLaunchKernelGGL(outlet_finish_kernel, dim3(nblocks), dim3(kBlock), 0, sm, h->out.table.p, (long long)n, h->cat.link.p, g.ncp, h->out.status.d);
    HIP_TRY(h->out.timer.mark(h->timing, 2, sm));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->out.status.h, h->out.status.d, sizeof(OutletStatus), hipMemcpyDeviceToHost, sm));
    if (wdpm_stream_sync(x, sm)) return 1;
    if (h->timing) HIP_TRY(h->out.timer.read_all());
  }
  if (h->out.status.h->deep)
    return wdpm_fail("wdpm_outlets_label: a cell of a pond's basin lies 512 m or more below the pond's outlet, or not a finite depth "
                     "below it: fill_q (a 64-bit sum of depths in units of 2^-24 m) is only safe below that depth");
  h->out.stats.ponds = n;
  h->out.stats.no_outlet = (int64_t)h->out.status.h->no_outlet;
  h->out.stats.to_land = (int64_t)h->out.status.h->to_land;
  h->out.stats.divide_cells = (int64_t)h->out.status.h->divide;
  h->out.valid = true;
  h->lab.valid = true;
  if (nponds) *nponds = n;
  return 0;
}

extern "C" int wdpm_outlets_table(wdpm_ponds *h, wdpm_pond_outlet *out, int64_t capacity) {
  return table_out("wdpm_outlets_table", h, &wdpm_ponds::out, kNoTable, out, capacity);
}

extern "C" int wdpm_outlets_stats(wdpm_ponds *h, wdpm_pond_outlet_stats *out) {
  return stats_out("wdpm_outlets_stats", h, &wdpm_ponds::out, kNoTable, out);
}

extern "C" int wdpm_outlets_phase_ms(wdpm_ponds *h, double *ms) {
  return phase_ms_out("wdpm_outlets_phase_ms", h, &wdpm_ponds::out, kNoTable, ms);
}

/* ---- row blocks (include/wdpm_group_pond_outlets.h) -------------------------------------------------------------------------- */
#include "wdpm_outlets_merge.h"

static_assert(sizeof(wdpm_outlets_merge::SlotRow) == sizeof(OutletRow) && offsetof(wdpm_outlets_merge::SlotRow, pair) == offsetof(OutletRow, pair) &&
              offsetof(wdpm_outlets_merge::SlotRow, to_basin) == offsetof(OutletRow, to_basin) &&
              offsetof(wdpm_outlets_merge::SlotRow, fill_q) == offsetof(OutletRow, fill_q), "the merge reads the slots' rows as the device leaves them");

namespace {
const char kNoGroupTable[] = "no outlet table: the last label call on this handle was not a wdpm_group_outlets_label that succeeded";

/* the rows beside the rank's own come as the catchment pass brought them */
OutRows rows_of(const wdpm_group_ponds *gh, int i) {
  const wdpm_ponds *h = gh->r[i];
  const OwnedRows own = owned_rows(gh, i);
  return {own.ra, own.rb, own.halo, h->cat.keys.p + (size_t)2 * h->g.ncp, h->rim.slot_of.p};
}

/* rank i's buffers for `slots` table rows; nothing is queued */
int group_outlets_buffers(wdpm_ponds *h, int i, long long slots) {
  HIP_TRY(hipSetDevice(h->x->p.device));
  const char *what;
  hipError_t e = ensure(h->out.status, &what);
  if (e != hipSuccess) return wdpm_fail("wdpm_group_outlets_label: no %s memory for the status words of rank %d: %s", what, i, hipGetErrorString(e));
  e = grow(h, h->out.h_seam, 2LL * h->g.ncp);
  if (e != hipSuccess) return wdpm_fail("wdpm_group_outlets_label: no pinned host memory for two rows of basins of rank %d: %s", i, hipGetErrorString(e));
  e = grow(h, h->out.table, slots);
  if (e != hipSuccess) return wdpm_fail("wdpm_group_outlets_label: no device memory for %lld outlet rows of rank %d: %s", slots, i, hipGetErrorString(e));
  if (2 * slots > h->out.keys.cap) { reset(h, h->out.keys); reset(h, h->out.h_keys); }   /* the two grow together: both go before either comes */
  e = grow(h, h->out.keys, 2 * slots);
  if (e != hipSuccess) return wdpm_fail("wdpm_group_outlets_label: no device memory for the pour keys of %lld slots of rank %d: %s", slots, i, hipGetErrorString(e));
  e = grow(h, h->out.h_keys, 3 * slots);
  if (e != hipSuccess) reset(h, h->out.keys);         /* neither without the other: the next call makes both again */
  if (e != hipSuccess) return wdpm_fail("wdpm_group_outlets_label: no pinned host memory for the pour keys of %lld slots of rank %d: %s", slots, i, hipGetErrorString(e));
  e = grow(h, h->out.h_table, slots);
  if (e != hipSuccess) return wdpm_fail("wdpm_group_outlets_label: no pinned host memory for %lld outlet rows of rank %d: %s", slots, i, hipGetErrorString(e));
  return 0;
}

/* one wait per rank that has work queued; the first message stays */
int group_outlets_wait(wdpm_group_ponds *gh, int ev_a, int ev_b, int phase) {
  bool bad = false;
  std::string first_msg;
  for (int i = 0; i < gh->n; i++) {
    wdpm_ponds *p = gh->r[i];
    if (p->cat.slots == 0) continue;
    bool failed = hipSetDevice(p->x->p.device) != hipSuccess || wdpm_stream_sync(p->x, p->x->stream);
    if (!failed && p->timing) {
      const hipError_t e = p->out.timer.read(ev_a, ev_b, &p->out.timer.ms[phase]);
      if (e != hipSuccess) failed = wdpm_fail("wdpm_group_outlets_label: the events of rank %d cannot be read: %s", i, hipGetErrorString(e)) != 0;
    }
    if (failed) {
      if (!bad) first_msg = wdpm_last_error();
      bad = true;
    }
  }
  return bad ? wdpm_fail("%s", first_msg.c_str()) : 0;
}
}  // namespace

extern "C" int wdpm_group_outlets_label(wdpm_group_ponds *h, double min_depth, int64_t *nponds) {
  if (!h) return wdpm_fail("wdpm_group_outlets_label: null handle");
  if (check_min_depth("wdpm_group_outlets_label", min_depth)) return 1;
  int64_t n = 0;
  const int rc = wdpm_group_catch_label(h, min_depth, &n);    /* leaves basins, seam keys, slots and the seam basins on the host */
  h->lab.valid = false;                                       /* a wdpm_group_outlets_label that fails leaves no table of any kind */
  if (rc) return 1;
  const int nr = h->n, ncp = h->ncp;
  for (int i = 0; i < nr; i++) {
    wdpm_ponds *p = h->r[i];
    p->out.timer.clear();
    if (n > 0 && p->cat.slots > 0 && group_outlets_buffers(p, i, p->cat.slots)) return 1;
  }
  h->out.rows.assign((size_t)n, wdpm_pond_outlet());
  wdpm_outlets_merge::Totals tot;
  double merge_ms = 0.0;
  if (n > 0) {                                                /* no pond, no outlet: nothing to launch */
    /* (A) every rank: the facing ranks' seam basins into its halo rows, init, passes, keys and divide counts on their way down */
    for (int i = 0; i < nr; i++) {
      wdpm_ponds *p = h->r[i];
      if (p->cat.slots == 0) continue;                      /* no basin > 0 in its rows: no pass starts there */
      wdpm_ctx *x = p->x;
      const Geom g = p->g;
      const hipStream_t sm = x->stream;
      const OutRows rw = rows_of(h, i);
      const long long slots = p->cat.slots;
      const size_t off = (size_t)p->row_off * g.ncp;
      const double *w = x->d_w[x->cur] + off, *dem = x->d_dem + off;
      const Waves wv = waves_for(p, rw.rb - rw.ra);
      const int rpw = wv.rpw, nwaves = wv.nwaves;
      hipError_t e = hipSetDevice(x->p.device);
      if (e == hipSuccess) e = hipMemsetAsync(p->out.status.d, 0, sizeof(OutletStatus), sm);
      if (e == hipSuccess) e = p->out.timer.mark(p->timing, 0, sm);
      for (int side = 0; side < 2 && e == hipSuccess; side++) {
        if (!(rw.halo & (1 << side))) continue;
        const int *src = side ? h->r[i + 1]->cat.h_exits.p : h->r[i - 1]->cat.h_exits.p + ncp;      /* the first row below, the last row above */
        memcpy(p->out.h_seam.p + (size_t)side * ncp, src, (size_t)ncp * sizeof(int));
        e = hipMemcpyAsync(p->cat.link.p + (size_t)(side ? g.rows - 1 : 0) * g.ncp, p->out.h_seam.p + (size_t)side * ncp, (size_t)ncp * sizeof(int),
                           hipMemcpyHostToDevice, sm);
      }
      if (e == hipSuccess) {
        hipLaunchKernelGGL(outlet_init_kernel, dim3(blocks_for(slots, kBlock)), dim3(kBlock), 0, sm, p->out.table.p, slots);
        hipLaunchKernelGGL(outlet_passes_rows_kernel, dim3(blocks_for(nwaves, kWaves)), dim3(kBlock), 0, sm, w, dem, p->cat.link.p, g, rpw, nwaves,
                           p->out.table.p, rw);
        hipLaunchKernelGGL(outlet_pour_down_kernel, dim3(blocks_for(slots, kBlock)), dim3(kBlock), 0, sm, p->out.table.p, slots, p->out.keys.p);
        e = hipGetLastError();
      }
      if (e == hipSuccess) e = p->out.timer.mark(p->timing, 1, sm);
      if (e == hipSuccess) e = hipMemcpyAsync(p->out.h_keys.p, p->out.keys.p, (size_t)2 * slots * sizeof(unsigned long long), hipMemcpyDeviceToHost, sm);
      if (e != hipSuccess) {
        (void)wdpm_fail("wdpm_group_outlets_label: queueing the passes of rank %d failed: %s", i, hipGetErrorString(e));
        return group_drain(h);
      }
    }
    if (group_outlets_wait(h, 0, 1, 0)) return 1;

    timespec t0, t1, t2, t3;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    std::vector<wdpm_outlets_merge::Rank> ranks((size_t)nr);
    std::vector<unsigned long long *> up((size_t)nr);
    for (int i = 0; i < nr; i++) {
      const wdpm_ponds *p = h->r[i];
      wdpm_outlets_merge::Rank &rk = ranks[(size_t)i];
      rk.label = p->rim.slot_label.data();
      rk.slots = p->cat.slots;
      rk.remote = p->cat.remote_label.data();
      rk.nremote = p->cat.remote;
      rk.key = p->out.h_keys.p;
      rk.divide = p->out.h_keys.p + p->cat.slots;
      rk.rows = reinterpret_cast<const wdpm_outlets_merge::SlotRow *>(p->out.h_table.p);
      rk.row_shift = h->view0[i];
      rk.own_lo = h->own_lo[i];
      rk.own_rows = h->own_rows[i];
      up[(size_t)i] = p->out.h_keys.p + 2 * p->cat.slots;       /* behind the 2 x slots words that came down */
    }
    std::vector<unsigned long long> pour_key((size_t)n);
    std::vector<long long> divide((size_t)n);
    std::string err;
    if (wdpm_outlets_merge::pour(ranks, n, pour_key.data(), divide.data(), up, err)) return wdpm_fail("wdpm_group_outlets_label: %s", err.c_str());
    clock_gettime(CLOCK_MONOTONIC, &t1);

    /* (B) every rank: the merged keys into its slots, locate, finish, its rows and its status word on their way down */
    for (int i = 0; i < nr; i++) {
      wdpm_ponds *p = h->r[i];
      if (p->cat.slots == 0) continue;
      wdpm_ctx *x = p->x;
      const Geom g = p->g;
      const hipStream_t sm = x->stream;
      const OutRows rw = rows_of(h, i);
      const long long slots = p->cat.slots;
      const size_t off = (size_t)p->row_off * g.ncp;
      const double *w = x->d_w[x->cur] + off, *dem = x->d_dem + off;
      const Waves wv = waves_for(p, rw.rb - rw.ra);
      const int rpw = wv.rpw, nwaves = wv.nwaves;
      hipError_t e = hipSetDevice(x->p.device);
      if (e == hipSuccess) e = p->out.timer.mark(p->timing, 1, sm);
      if (e == hipSuccess) e = hipMemcpyAsync(p->out.keys.p, up[(size_t)i], (size_t)slots * sizeof(unsigned long long), hipMemcpyHostToDevice, sm);
      if (e == hipSuccess) {
        hipLaunchKernelGGL(outlet_pour_up_kernel, dim3(blocks_for(slots, kBlock)), dim3(kBlock), 0, sm, p->out.table.p, slots, p->out.keys.p);
        hipLaunchKernelGGL(outlet_locate_rows_kernel, dim3(blocks_for(nwaves, kWaves)), dim3(kBlock), 0, sm, w, dem, p->cat.link.p, g, rpw, nwaves,
                           p->out.table.p, p->out.status.d, rw);
        hipLaunchKernelGGL(outlet_finish_rows_kernel, dim3(blocks_for(slots, kBlock)), dim3(kBlock), 0, sm, p->out.table.p, slots, p->cat.link.p, g.ncp);
        e = hipGetLastError();
      }
      if (e == hipSuccess) e = p->out.timer.mark(p->timing, 2, sm);
      if (e == hipSuccess) e = hipMemcpyAsync(p->out.h_table.p, p->out.table.p, (size_t)slots * sizeof(OutletRow), hipMemcpyDeviceToHost, sm);
      if (e == hipSuccess) e = hipMemcpyAsync(p->out.status.h, p->out.status.d, sizeof(OutletStatus), hipMemcpyDeviceToHost, sm);
      if (e != hipSuccess) {
        (void)wdpm_fail("wdpm_group_outlets_label: queueing the locate pass of rank %d failed: %s", i, hipGetErrorString(e));
        return group_drain(h);
      }
    }
    if (group_outlets_wait(h, 1, 2, 1)) return 1;
    for (int i = 0; i < nr; i++)
      if (h->r[i]->cat.slots > 0 && h->r[i]->out.status.h->deep)
        return wdpm_fail("wdpm_group_outlets_label: a cell of a pond's basin in the rows of rank %d lies 512 m or more below the pond's outlet, or "
                         "not a finite depth below it: fill_q (a 64-bit sum of depths in units of 2^-24 m) is only safe below that depth", i);

    clock_gettime(CLOCK_MONOTONIC, &t2);
    if (wdpm_outlets_merge::merge(ranks, n, ncp, pour_key.data(), divide.data(), h->out.rows.data(), tot, err))
      return wdpm_fail("wdpm_group_outlets_label: %s", err.c_str());
    clock_gettime(CLOCK_MONOTONIC, &t3);
    merge_ms = ms_between(t0, t1) + ms_between(t2, t3);
  }
  h->out.stats.ponds = n;
  h->out.stats.no_outlet = tot.no_outlet;
  h->out.stats.to_land = tot.to_land;
  h->out.stats.divide_cells = tot.divide_cells;
  h->out.stats.ranks = nr;
  h->out.stats.seam_outlets = tot.seam_outlets;
  h->out.stats.split_ponds = tot.split_ponds;
  h->out.stats.merge_ms = merge_ms;
  h->out.valid = true;
  h->lab.valid = true;
  if (nponds) *nponds = n;
  return 0;
}

extern "C" int wdpm_group_outlets_table(wdpm_group_ponds *h, wdpm_pond_outlet *out, int64_t capacity) {
  return table_out("wdpm_group_outlets_table", h, &wdpm_group_ponds::out, kNoGroupTable, out, capacity);
}

extern "C" int wdpm_group_outlets_stats(wdpm_group_ponds *h, wdpm_group_outlet_stats *out) {
  return stats_out("wdpm_group_outlets_stats", h, &wdpm_group_ponds::out, kNoGroupTable, out);
}

extern "C" int wdpm_group_outlets_phase_ms(wdpm_group_ponds *h, int32_t rank, double *ms) {
  return group_phase_ms_out("wdpm_group_outlets_phase_ms", h, &wdpm_group_ponds::out, &wdpm_ponds::out, kNoGroupTable, rank, ms);
}
#endif  /* WDPM_PONDS_EMULATION */
