/*
 * wdpm_pond_rims.hip — the rim of every pond (include/wdpm_pond_rims.h): spill level and where it lies, shoreline, walls and the
 * spread of the water surface, from the label raster, the wet masks, the DEM and the water a label call leaves on the device.
 * gfx950.  A unit of its own beside wdpm_ponds.hip: not in the launch ledger, not among the sources wdpm_build_info() hashes.
 *
 * Shaped like the table kernel: a wave owns one 64-column segment over rows_per_wave rows (ponds_rows_per_wave).
 *
 *   rim      The wet masks say without a label which dry lanes have a wet neighbour: the three rows' masks, each widened by one
 *            column either way (with the edge bits of the segments left and right), minus the row's own mask.  Rows whose three
 *            masks are empty take no work; a row without such lanes reads dem and w of its pond cells only.  Labels live in a
 *            sliding three-row window in registers, read for wet lanes only (a dry lane's label is 0 by its mask) and only when a
 *            row needs them; a row whose mask equals the mask above it has the labels above it.  Column neighbours come from the
 *            lanes next door, those of lanes 0 and 63 from memory.  A neighbour lane gathers its distinct labels (four at most:
 *            two neighbours that touch each other lie in one pond), a pond lane gives depth_key(dem + w) to its own.  Then per
 *            wave BY LABEL: ballots of the lanes that hold label L, popcounts for the two counts, min / max over the lanes' keys;
 *            carried down the rows while the label stays, and one set of atomics per (wave, label change)
 *   locate   the same walk over the rows that have neighbour lanes: a rim lane whose level key equals its pond's final rim key
 *            offers its padded index (atomicMin on an int32: a view holds fewer than 2^31 cells)
 *   finish   keys back to doubles, the index to row and column; +inf, -1, -1 for a pond without rim cells
 *
 * Over row blocks (include/wdpm_group_pond_rims.h) every rank runs the same body over its owned rows, with the whole-raster labels
 * of the one row beyond either end uploaded beside them and its table indexed through a flat label -> slot table (rim_slot,
 * rims_slots_kernel); the host merges the ranks' rows (wdpm_rims_merge.h).
 *
 * tests/rims_emu_main.cpp and tests/group_rims_emu_main.cpp compile the kernels for the host under sanitizers with
 * WDPM_PONDS_EMULATION defined, as tests/ponds_emu_main.cpp does with wdpm_ponds.hip, and leave the host half out.
 */
#include "wdpm_ponds_priv.h"

using namespace wdpm_pond_detail;

namespace {

/* one row of the window: the masks of the segment and of its neighbours, the labels of the wet lanes (0 elsewhere) and of the two
 * cells beside the segment.  Everything but lbl is wave-uniform. */
struct RimWin {
  unsigned long long m, ml, mr;
  int lbl, el, er;
  bool has_lbl, has_edges;
};

/* a mask widened by one column either way, with the edge bits of the neighbouring segments */
__device__ __forceinline__ unsigned long long widen(const RimWin &w) {
  return w.m | (w.m << 1) | (w.m >> 1) | (w.ml >> 63) | ((w.mr & 1ull) << 63);
}

/* the masks of row r (empty outside the raster); nothing of the labels yet */
__device__ __forceinline__ RimWin win_open(const unsigned long long *__restrict__ masks, const Geom &g, int r, int s) {
  RimWin w;
  w.m = w.ml = w.mr = 0ull;
  w.lbl = w.el = w.er = 0;
  w.has_lbl = w.has_edges = false;
  if (r >= 0 && r < g.rows) {
    const unsigned long long *row = masks + (long long)r * g.nsc;
    w.m = row[s];
    if (s > 0) w.ml = row[s - 1];
    if (s < g.nsc - 1) w.mr = row[s + 1];
  }
  return w;
}

/* the labels of row r's wet lanes; `above` is the row above it in the window */
__device__ __forceinline__ void win_labels(RimWin &w, const RimWin &above, const int *__restrict__ labels, const Geom &g, int r,
                                           int c, int lane) {
  if (w.has_lbl) return;
  if (w.m == 0ull) w.lbl = 0;
  else if (above.has_lbl && above.m == w.m) w.lbl = above.lbl;      /* every run lies under the same run */
  else w.lbl = bit(w.m, lane) ? labels[r * g.ncp + c] : 0;
  w.has_lbl = true;
}

/* ... and of the cells left and right of the segment (a set edge bit says that the cell exists and is wet) */
__device__ __forceinline__ void win_edges(RimWin &w, const int *__restrict__ labels, const Geom &g, int r, int s) {
  if (w.has_edges) return;
  w.el = (w.ml >> 63) ? labels[r * g.ncp + s * kSeg - 1] : 0;
  w.er = (w.mr & 1ull) ? labels[r * g.ncp + s * kSeg + kSeg] : 0;
  w.has_edges = true;
}

/* what a wave has gathered for one label and not yet sent */
struct RimCarry {
  int label;               /* 0: nothing held */
  unsigned long long smin, smax, rmin, rim_cells, wall_cells;
};

__device__ __forceinline__ void rim_carry_reset(RimCarry &c, int label) {
  c.label = label;
  c.smin = c.rmin = ~0ull;
  c.smax = 0ull;
  c.rim_cells = c.wall_cells = 0ull;
}

/* The table row of label L: row L - 1 of a whole raster's table.  kSlots (row blocks): the labels are whole-raster numbers and the
 * table holds one row per pond the rank touches, so slot_of[L] says which (wdpm_group_rims_label fills it). */
template <bool kSlots>
__device__ __forceinline__ int rim_slot(const int *__restrict__ slot_of, int L) {
  return kSlots ? slot_of[L] : L - 1;
}

/* one lane sends a carry: the extrema through atomic_min_if / atomic_max_if */
template <bool kSlots>
__device__ __forceinline__ void rim_send(RimRow *table, const int *__restrict__ slot_of, const RimCarry &c) {
  RimRow *t = table + rim_slot<kSlots>(slot_of, c.label);
  atomic_min_if(&t->smin_key, c.smin);
  atomic_max_if(&t->smax_key, c.smax);
  atomic_min_if(&t->rim_key, c.rmin);
  if (c.rim_cells) atomicAdd(&t->rim_cells, c.rim_cells);
  if (c.wall_cells) atomicAdd(&t->wall_cells, c.wall_cells);
}

/* kLocate false: the rim pass.  kLocate true: the locate pass, after every rim key is final.  Everything that steers the loops
 * is wave-uniform.  The strips are cut over rows [ra, rb) of the view: all of a whole raster; the owned rows of a row block, whose
 * view rows 0 and g.rows - 1 then only ever stand above or below a strip, with the masks and labels of the neighbouring rank's
 * row (nothing of their dem or water is read).  kSlots: see rim_slot. */
template <bool kLocate, bool kSlots>
__device__ __forceinline__ void rims_body(const double *__restrict__ w, const double *__restrict__ dem,
                                          const unsigned long long *__restrict__ masks, const int *__restrict__ labels, const Geom g,
                                          const int rpw, const int nwaves, RimRow *table, const int ra, const int rb,
                                          const int *__restrict__ slot_of) {
  const int wid = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (wid >= nwaves) return;
  const int lane = threadIdx.x & 63;
  const int strip = wid / g.nsc, s = wid - strip * g.nsc;
  const int r0 = ra + strip * rpw, r1 = min(r0 + rpw, rb);
  const int c = s * kSeg + lane;
  RimCarry cy;
  rim_carry_reset(cy, 0);

  RimWin up = win_open(masks, g, r0 - 1, s), cur = win_open(masks, g, r0, s), dn;
  for (int r = r0; r < r1; r++, up = cur, cur = dn) {
    dn = win_open(masks, g, r + 1, s);
    const unsigned long long nbm = (widen(up) | widen(cur) | widen(dn)) & ~cur.m;   /* dry lanes with a wet neighbour */
    if (kLocate ? nbm == 0ull : (nbm | cur.m) == 0ull) continue;
    const bool wet = bit(cur.m, lane), nb = bit(nbm, lane);
    const int idx = r * g.ncp + c;         /* read by wet and nb lanes only: their columns lie inside the raster */

    /* this lane's labels: its own (a pond lane) or those of the ponds around it (a neighbour lane), each once */
    int q0 = 0, q1 = 0, q2 = 0, q3 = 0;
    if (!kLocate || nbm) win_labels(cur, up, labels, g, r, c, lane);
    if (nbm) {
      win_labels(up, up, labels, g, r - 1, c, lane);     /* (no row above it in the window: read) */
      win_labels(dn, cur, labels, g, r + 1, c, lane);
      win_edges(up, labels, g, r - 1, s);
      win_edges(cur, labels, g, r, s);
      win_edges(dn, labels, g, r + 1, s);
      const int around[8] = {lane_from_left(up.lbl, up.el, lane),  up.lbl,  lane_from_right(up.lbl, up.er, lane),
                             lane_from_left(cur.lbl, cur.el, lane),         lane_from_right(cur.lbl, cur.er, lane),
                             lane_from_left(dn.lbl, dn.el, lane),  dn.lbl,  lane_from_right(dn.lbl, dn.er, lane)};
      if (nb) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const int v = around[i];
          if (v != 0 && v != q0 && v != q1 && v != q2 && v != q3) {
            if (q0 == 0) q0 = v;
            else if (q1 == 0) q1 = v;
            else if (q2 == 0) q2 = v;
            else q3 = v;
          }
        }
      }
    }
    if (wet) q0 = cur.lbl;

    unsigned long long key = 0ull;         /* a pond lane's surface, a neighbour lane's level */
    bool wall = false;
    if (kLocate ? nb : (wet || nb)) {
      const double e = dem[idx], d = w[idx];
      wall = !(e < __builtin_inf());
      key = depth_key((wet || d > 0.0) ? e + d : e);
    }

    if (kLocate) {
      if (nb && !wall) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int L = i == 0 ? q0 : i == 1 ? q1 : i == 2 ? q2 : q3;
          if (L == 0) continue;
          RimRow *t = table + rim_slot<kSlots>(slot_of, L);
          if (t->rim_key == key && __hip_atomic_load(&t->rim_idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > idx)
            atomicMin(&t->rim_idx, idx);
        }
      }
      continue;
    }

    /* per wave, by label */
    for (;;) {
      const int cand = q0 ? q0 : q1 ? q1 : q2 ? q2 : q3;
      const unsigned long long pending = __ballot(cand != 0);
      if (pending == 0ull) break;
      const int L = __shfl(cand, __builtin_ctzll(pending));
      const bool hit = q0 == L || q1 == L || q2 == L || q3 == L;
      const unsigned long long pondm = __ballot(hit && wet);
      const unsigned long long rimm = __ballot(hit && !wet && !wall);
      const unsigned long long wallm = __ballot(hit && !wet && wall);
      if (cy.label != L) {                  /* down the rows: the same label goes on gathering, another one sends first */
        if (cy.label != 0 && lane == 0) rim_send<kSlots>(table, slot_of, cy);
        rim_carry_reset(cy, L);
      }
      if (pondm) {
        const unsigned long long lo = wave_min(hit && wet ? key : ~0ull), hi = wave_max(hit && wet ? key : 0ull);
        cy.smin = lo < cy.smin ? lo : cy.smin;
        cy.smax = hi > cy.smax ? hi : cy.smax;
      }
      if (rimm) {
        const unsigned long long lo = wave_min(hit && !wet && !wall ? key : ~0ull);
        cy.rmin = lo < cy.rmin ? lo : cy.rmin;
        cy.rim_cells += (unsigned long long)__popcll(rimm);
      }
      cy.wall_cells += (unsigned long long)__popcll(wallm);
      if (q0 == L) q0 = 0;
      if (q1 == L) q1 = 0;
      if (q2 == L) q2 = 0;
      if (q3 == L) q3 = 0;
    }
  }
  if (!kLocate && cy.label != 0 && lane == 0) rim_send<kSlots>(table, slot_of, cy);
}

__global__ __launch_bounds__(kBlock) void rims_pass_kernel(const double *__restrict__ w, const double *__restrict__ dem,
                                                           const unsigned long long *__restrict__ masks,
                                                           const int *__restrict__ labels, Geom g, int rpw, int nwaves,
                                                           RimRow *table) {
  rims_body<false, false>(w, dem, masks, labels, g, rpw, nwaves, table, 0, g.rows, nullptr);
}

__global__ __launch_bounds__(kBlock) void rims_locate_kernel(const double *__restrict__ w, const double *__restrict__ dem,
                                                             const unsigned long long *__restrict__ masks,
                                                             const int *__restrict__ labels, Geom g, int rpw, int nwaves,
                                                             RimRow *table) {
  rims_body<true, false>(w, dem, masks, labels, g, rpw, nwaves, table, 0, g.rows, nullptr);
}

/* the same two passes over the owned rows [ra, rb) of a row block's view, the table indexed through slot_of */
__global__ __launch_bounds__(kBlock) void rims_pass_rows_kernel(const double *__restrict__ w, const double *__restrict__ dem,
                                                                const unsigned long long *__restrict__ masks,
                                                                const int *__restrict__ labels, Geom g, int rpw, int nwaves,
                                                                RimRow *table, int ra, int rb, const int *__restrict__ slot_of) {
  rims_body<false, true>(w, dem, masks, labels, g, rpw, nwaves, table, ra, rb, slot_of);
}

__global__ __launch_bounds__(kBlock) void rims_locate_rows_kernel(const double *__restrict__ w, const double *__restrict__ dem,
                                                                  const unsigned long long *__restrict__ masks,
                                                                  const int *__restrict__ labels, Geom g, int rpw, int nwaves,
                                                                  RimRow *table, int ra, int rb, const int *__restrict__ slot_of) {
  rims_body<true, true>(w, dem, masks, labels, g, rpw, nwaves, table, ra, rb, slot_of);
}

/* slot_of for one rank (every entry INT_MAX before): local pond l (map[l - 1] in the whole raster) has slot l - 1, and local ponds
 * that are one pond of the whole raster share the slot of the first of them; foreign pond j, which the host found in the rows
 * beside the rank's own and in none of its cells, has slot nlocal + j.  The two kinds never meet in one entry. */
__global__ __launch_bounds__(kBlock) void rims_slots_kernel(const int *__restrict__ map, int nlocal, const int *__restrict__ foreign,
                                                            int nforeign, int *slot_of) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < nlocal) atomicMin(&slot_of[map[i]], i);
  else if (i - nlocal < nforeign) slot_of[foreign[i - nlocal]] = i;
}

__global__ __launch_bounds__(kBlock) void rims_init_kernel(RimRow *t, long long n) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  RimRow r;
  r.smin_key = r.rim_key = ~0ull;
  r.smax_key = 0ull;
  r.rim_idx = INT_MAX;
  r.pad = 0;
  r.rim_cells = r.wall_cells = 0ull;
  t[i] = r;
}

/* the accumulated row becomes a wdpm_pond_rim in place */
__global__ __launch_bounds__(kBlock) void rims_finish_kernel(RimRow *t, long long n, int ncp) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  RimRow r = t[i];
  const bool rim = r.rim_cells != 0ull && r.rim_idx != INT_MAX;
  r.smin_key = (unsigned long long)__double_as_longlong(depth_from_key(r.smin_key));
  r.smax_key = (unsigned long long)__double_as_longlong(depth_from_key(r.smax_key));
  r.rim_key = (unsigned long long)__double_as_longlong(rim ? depth_from_key(r.rim_key) : __builtin_inf());
  const int row = rim ? r.rim_idx / ncp : -1;
  r.pad = rim ? r.rim_idx - row * ncp : -1;     /* rim_col */
  r.rim_idx = row;                              /* rim_row */
  t[i] = r;
}

}  // namespace

#ifndef WDPM_PONDS_EMULATION
/* ---- host ------------------------------------------------------------------------------------------------------------------ */
extern "C" int wdpm_rims_label(wdpm_ponds *h, double min_depth, int64_t *nponds) {
  if (!h) return wdpm_fail("wdpm_rims_label: null handle");
  if (check_min_depth("wdpm_rims_label", min_depth)) return 1;
  if (h->seams) return wdpm_fail("wdpm_rims_label: the handle views a row block: rims are taken on whole rasters only");
  int64_t n = 0;
  if (wdpm_ponds_label(h, min_depth, &n)) return 1;           /* leaves masks, labels and the stream as the rim pass wants them */
  wdpm_ctx *x = h->x;
  const Geom g = h->g;
  const hipStream_t sm = x->stream;
  HIP_TRY(hipSetDevice(x->p.device));
  const hipError_t e = grow(h, h->rim.table, n);              /* sized from N, like the pond table */
  if (e != hipSuccess) return wdpm_fail("wdpm_rims_label: no device memory for the rims of %lld ponds: %s", (long long)n, hipGetErrorString(e));
  h->rim.timer.clear();
  if (n > 0) {                                                /* no pond, no rim: nothing to launch */
    const size_t off = (size_t)h->row_off * g.ncp;
    const double *w = x->d_w[x->cur] + off, *dem = x->d_dem + off;
    const Waves wv = waves_for(h, g.rows);
    const int rpw = wv.rpw, nwaves = wv.nwaves;
    const unsigned nblocks = blocks_for(n, kBlock), wblocks = blocks_for(nwaves, kWaves);
    HIP_TRY(h->rim.timer.mark(h->timing, 0, sm));
    hipLaunchKernelGGL(rims_init_kernel, dim3(nblocks), dim3(kBlock), 0, sm, h->rim.table.p, (long long)n);
    hipLaunchKernelGGL(rims_pass_kernel, dim3(wblocks), dim3(kBlock), 0, sm, w, dem, h->lab.masks.p, h->lab.labels.p, g, rpw, nwaves, h->rim.table.p);
    HIP_TRY(h->rim.timer.mark(h->timing, 1, sm));
    hipLaunchKernelGGL(rims_locate_kernel, dim3(wblocks), dim3(kBlock), 0, sm, w, dem, h->lab.masks.p, h->lab.labels.p, g, rpw, nwaves, h->rim.table.p);
    hipLaunchKernelGGL(rims_finish_kernel, dim3(nblocks), dim3(kBlock), 0, sm, h->rim.table.p, (long long)n, g.ncp);
    HIP_TRY(h->rim.timer.mark(h->timing, 2, sm));
    HIP_TRY(hipGetLastError());
    if (wdpm_stream_sync(x, sm)) return 1;
    if (h->timing) HIP_TRY(h->rim.timer.read_all());
  }
  h->rim.valid = true;
  if (nponds) *nponds = n;
  return 0;
}

namespace {
const char kNoTable[] = "no rim table: the last label call on this handle was not a wdpm_rims_label that succeeded";
const char kNoGroupTable[] = "no rim table: the last label call on this handle was not a wdpm_group_rims_label that succeeded";
}  // namespace

extern "C" int wdpm_rims_table(wdpm_ponds *h, wdpm_pond_rim *out, int64_t capacity) {
  return table_out("wdpm_rims_table", h, &wdpm_ponds::rim, kNoTable, out, capacity);
}

extern "C" int wdpm_rims_phase_ms(wdpm_ponds *h, double *ms) {
  return phase_ms_out("wdpm_rims_phase_ms", h, &wdpm_ponds::rim, kNoTable, ms, true);
}

/* ---- row blocks (include/wdpm_group_pond_rims.h) ----------------------------------------------------------------------------- */
#include "wdpm_rims_merge.h"

/* Rank i's rim work behind its table kernels, on its stream, nothing waited for (group_label calls this for every rank before the
 * first wait).  The rows beside the rank's own come from the neighbours' seam rows through the stitch's numbers. */
int wdpm_pond_detail::group_rims_rank(wdpm_group_ponds *gh, int i, const std::vector<std::vector<int>> &map, long long ponds) {
  wdpm_ponds *h = gh->r[i];
  wdpm_ctx *x = h->x;
  const Geom g = h->g;
  const hipStream_t sm = x->stream;
  const int ncp = g.ncp, nsc = g.nsc;
  const bool up = i > 0, dn = i + 1 < gh->n;
  h->rim.timer.clear();
  h->rim.slots = h->rim.nforeign = 0;
  h->rim.slot_label.clear();
  if (ponds == 0) return 0;
  HIP_TRY(hipSetDevice(x->p.device));
  hipError_t e = grow(h, h->rim.h_beside, 2LL * nsc + 2LL * ncp);     /* 2 x nsc masks, then 4 x ncp ints in the place of 2 x ncp words */
  if (e != hipSuccess) return wdpm_fail("wdpm_group_rims_label: no pinned host memory for two rows: %s", hipGetErrorString(e));
  e = grow(h, h->rim.foreign, 2LL * ncp);
  if (e != hipSuccess) return wdpm_fail("wdpm_group_rims_label: no device memory for two rows of labels: %s", hipGetErrorString(e));
  unsigned long long *bm = h->rim.h_beside.p;             /* [2][nsc] */
  int *bl = (int *)(bm + (size_t)2 * nsc);          /* [2][ncp] */
  int *bf = bl + (size_t)2 * ncp;                   /* up to 2 * ncp foreign labels */
  memset(bm, 0, (size_t)2 * nsc * sizeof(unsigned long long));
  memset(bl, 0, (size_t)2 * ncp * sizeof(int));
  for (int side = 0; side < 2; side++) {
    if (side ? !dn : !up) continue;
    const int j = side ? i + 1 : i - 1;
    const int *src = gh->r[j]->lab.h_seam.p + (side ? 0 : ncp);     /* the lower rank's first owned row, the upper rank's last */
    for (int c = 0; c < ncp; c++)
      if (src[c]) {
        bl[side * ncp + c] = map[j][(size_t)src[c] - 1];
        bm[side * nsc + c / kSeg] |= 1ull << (c % kSeg);
      }
  }
  std::vector<int> own, foreign;
  for (int side = 0; side < 2; side++) {
    if (side ? !dn : !up) continue;
    const int *src = h->lab.h_seam.p + side * ncp;
    for (int c = 0; c < ncp; c++)
      if (src[c]) own.push_back(map[i][(size_t)src[c] - 1]);
  }
  wdpm_rims_merge::foreign_labels(bl, (size_t)2 * ncp, own.data(), own.size(), foreign);
  const long long nlocal = (long long)map[i].size(), nforeign = (long long)foreign.size(), slots = nlocal + nforeign;
  if (slots == 0) return 0;                         /* no pond in the rank's rows, none beside them */
  if (slots > (long long)0x7f7f7f7f) return wdpm_fail("wdpm_group_rims_label: rank %d would hold %lld rim rows", i, slots);
  for (long long k = 0; k < nforeign; k++) bf[k] = foreign[(size_t)k];
  h->rim.slot_label = map[i];
  h->rim.slot_label.insert(h->rim.slot_label.end(), foreign.begin(), foreign.end());

  e = grow(h, h->rim.table, slots);
  if (e != hipSuccess) return wdpm_fail("wdpm_group_rims_label: no device memory for the rims of %lld ponds: %s", slots, hipGetErrorString(e));
  e = grow(h, h->rim.slot_of, ponds + 1);
  if (e != hipSuccess) return wdpm_fail("wdpm_group_rims_label: no device memory for the slots of %lld ponds: %s", ponds, hipGetErrorString(e));
  e = grow(h, h->rim.h_table, slots);
  if (e != hipSuccess) return wdpm_fail("wdpm_group_rims_label: no pinned host memory for %lld rim rows: %s", slots, hipGetErrorString(e));

  /* the rows beside the rank's own, into view rows 0 and g.rows - 1, which the label path left dry and unlabelled */
  for (int side = 0; side < 2; side++) {
    if (side ? !dn : !up) continue;
    const size_t row = side ? (size_t)g.rows - 1 : 0;
    HIP_TRY(hipMemcpyAsync(h->lab.labels.p + row * ncp, bl + (size_t)side * ncp, (size_t)ncp * sizeof(int), hipMemcpyHostToDevice, sm));
    HIP_TRY(hipMemcpyAsync(h->lab.masks.p + row * nsc, bm + (size_t)side * nsc, (size_t)nsc * sizeof(unsigned long long), hipMemcpyHostToDevice, sm));
  }
  if (nforeign) HIP_TRY(hipMemcpyAsync(h->rim.foreign.p, bf, (size_t)nforeign * sizeof(int), hipMemcpyHostToDevice, sm));

  const size_t off = (size_t)h->row_off * ncp;
  const double *w = x->d_w[x->cur] + off, *dem = x->d_dem + off;
  const OwnedRows orw = owned_rows(gh, i);
  const int ra = orw.ra, rb = orw.rb;                 /* the owned rows, in rows of the view */
  const Waves wv = waves_for(h, rb - ra);
  const int rpw = wv.rpw, nwaves = wv.nwaves;
  const unsigned sblocks = blocks_for(slots, kBlock), wblocks = blocks_for(nwaves, kWaves);
  HIP_TRY(h->rim.timer.mark(h->timing, 0, sm));
  /* every entry above any slot (slots <= 0x7f7f7f7f); only the entries of the rank's own and foreign ponds are ever read */
  HIP_TRY(hipMemsetAsync(h->rim.slot_of.p, 0x7f, (size_t)(ponds + 1) * sizeof(int), sm));
  hipLaunchKernelGGL(rims_slots_kernel, dim3(sblocks), dim3(kBlock), 0, sm, h->lab.map.p, (int)nlocal, h->rim.foreign.p, (int)nforeign, h->rim.slot_of.p);
  hipLaunchKernelGGL(rims_init_kernel, dim3(sblocks), dim3(kBlock), 0, sm, h->rim.table.p, slots);
  hipLaunchKernelGGL(rims_pass_rows_kernel, dim3(wblocks), dim3(kBlock), 0, sm, w, dem, h->lab.masks.p, h->lab.labels.p, g, rpw, nwaves, h->rim.table.p,
                     ra, rb, h->rim.slot_of.p);
  HIP_TRY(h->rim.timer.mark(h->timing, 1, sm));
  hipLaunchKernelGGL(rims_locate_rows_kernel, dim3(wblocks), dim3(kBlock), 0, sm, w, dem, h->lab.masks.p, h->lab.labels.p, g, rpw, nwaves, h->rim.table.p,
                     ra, rb, h->rim.slot_of.p);
  hipLaunchKernelGGL(rims_finish_kernel, dim3(sblocks), dim3(kBlock), 0, sm, h->rim.table.p, slots, ncp);
  HIP_TRY(h->rim.timer.mark(h->timing, 2, sm));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h->rim.h_table.p, h->rim.table.p, (size_t)slots * sizeof(wdpm_pond_rim), hipMemcpyDeviceToHost, sm));
  h->rim.slots = slots;
  h->rim.nforeign = nforeign;
  return 0;
}

/* after group_label(.., group_rims_rank) has returned: the ranks' rim rows into h->rim.rows */
int wdpm_pond_detail::group_rims_merge(wdpm_group_ponds *h, const char *caller, long long n) {
  h->lab.valid = false;                                                 /* until the rims are merged as well */
  std::vector<wdpm_rims_merge::RankRims> ranks((size_t)h->n);
  long long slots = 0, foreign = 0;
  for (int i = 0; i < h->n; i++) {
    wdpm_ponds *p = h->r[i];
    if (h->timing && p->rim.slots > 0) {
      HIP_TRY(hipSetDevice(p->x->p.device));
      HIP_TRY(p->rim.timer.read_all());
    }
    ranks[(size_t)i] = {p->rim.h_table.p, p->rim.slot_label.data(), p->rim.slots, h->view0[i]};
    slots += p->rim.slots;
    foreign += p->rim.nforeign;
  }
  timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  h->rim.rows.resize((size_t)n);
  std::string err;
  if (wdpm_rims_merge::merge(ranks, n, h->rim.rows.data(), err)) return wdpm_fail("%s: %s", caller, err.c_str());
  clock_gettime(CLOCK_MONOTONIC, &t1);
  h->rim.stats.ranks = h->n;
  h->rim.stats.slots = slots;
  h->rim.stats.foreign = foreign;
  h->rim.stats.merge_ms = ms_between(t0, t1);
  h->lab.valid = true;
  h->rim.valid = true;
  return 0;
}

extern "C" int wdpm_group_rims_label(wdpm_group_ponds *h, double min_depth, int64_t *nponds) {
  if (!h) return wdpm_fail("wdpm_group_rims_label: null handle");
  if (check_min_depth("wdpm_group_rims_label", min_depth)) return 1;
  int64_t n = 0;
  if (group_label(h, min_depth, &n, group_rims_rank)) return 1;       /* every stream has run dry: one wait per rank ended both tables */
  if (group_rims_merge(h, "wdpm_group_rims_label", n)) return 1;
  if (nponds) *nponds = n;
  return 0;
}

extern "C" int wdpm_group_rims_table(wdpm_group_ponds *h, wdpm_pond_rim *out, int64_t capacity) {
  return table_out("wdpm_group_rims_table", h, &wdpm_group_ponds::rim, kNoGroupTable, out, capacity);
}

extern "C" int wdpm_group_rims_stats(wdpm_group_ponds *h, wdpm_group_rim_stats *out) {
  return stats_out("wdpm_group_rims_stats", h, &wdpm_group_ponds::rim, kNoGroupTable, out, true);
}

extern "C" int wdpm_group_rims_phase_ms(wdpm_group_ponds *h, int32_t rank, double *ms) {
  return group_phase_ms_out("wdpm_group_rims_phase_ms", h, &wdpm_group_ponds::rim, &wdpm_ponds::rim, kNoGroupTable, rank, ms, true);
}
#endif  /* WDPM_PONDS_EMULATION */
