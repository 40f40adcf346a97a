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
 * tests/rims_emu_main.cpp compiles the kernels for the host under sanitizers with WDPM_PONDS_EMULATION defined, as
 * tests/ponds_emu_main.cpp does with wdpm_ponds.hip, and leaves the host half out.
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

__device__ __forceinline__ int from_left(int v, int edge, int lane) {
  const int t = __shfl_up(v, 1);
  return lane > 0 ? t : edge;
}
__device__ __forceinline__ int from_right(int v, int edge, int lane) {
  const int t = __shfl_down(v, 1);
  return lane < 63 ? t : edge;
}

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

/* one lane sends a carry.  The extrema only move one way, so a look first spares the atomic that would change nothing; what a
 * carry never gathered still holds its start value and passes no look. */
__device__ __forceinline__ void rim_send(RimRow *table, const RimCarry &c) {
  RimRow *t = table + (c.label - 1);
  if (__hip_atomic_load(&t->smin_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > c.smin) atomicMin(&t->smin_key, c.smin);
  if (__hip_atomic_load(&t->smax_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < c.smax) atomicMax(&t->smax_key, c.smax);
  if (__hip_atomic_load(&t->rim_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > c.rmin) atomicMin(&t->rim_key, c.rmin);
  if (c.rim_cells) atomicAdd(&t->rim_cells, c.rim_cells);
  if (c.wall_cells) atomicAdd(&t->wall_cells, c.wall_cells);
}

/* kLocate false: the rim pass.  kLocate true: the locate pass, after every rim key is final.  Everything that steers the loops
 * is wave-uniform. */
template <bool kLocate>
__device__ __forceinline__ void rims_body(const double *__restrict__ w, const double *__restrict__ dem,
                                          const unsigned long long *__restrict__ masks, const int *__restrict__ labels, const Geom g,
                                          const int rpw, const int nwaves, RimRow *table) {
  const int wid = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (wid >= nwaves) return;
  const int lane = threadIdx.x & 63;
  const int rb = wid / g.nsc, s = wid - rb * g.nsc;
  const int r0 = rb * rpw, r1 = min(r0 + rpw, g.rows);
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
      const int around[8] = {from_left(up.lbl, up.el, lane),  up.lbl,  from_right(up.lbl, up.er, lane),
                             from_left(cur.lbl, cur.el, lane),         from_right(cur.lbl, cur.er, lane),
                             from_left(dn.lbl, dn.el, lane),  dn.lbl,  from_right(dn.lbl, dn.er, lane)};
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
          if (L != 0 && table[L - 1].rim_key == key &&
              __hip_atomic_load(&table[L - 1].rim_idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > idx)
            atomicMin(&table[L - 1].rim_idx, idx);
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
        if (cy.label != 0 && lane == 0) rim_send(table, cy);
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
  if (!kLocate && cy.label != 0 && lane == 0) rim_send(table, cy);
}

__global__ __launch_bounds__(kBlock) void rims_pass_kernel(const double *__restrict__ w, const double *__restrict__ dem,
                                                           const unsigned long long *__restrict__ masks,
                                                           const int *__restrict__ labels, Geom g, int rpw, int nwaves,
                                                           RimRow *table) {
  rims_body<false>(w, dem, masks, labels, g, rpw, nwaves, table);
}

__global__ __launch_bounds__(kBlock) void rims_locate_kernel(const double *__restrict__ w, const double *__restrict__ dem,
                                                             const unsigned long long *__restrict__ masks,
                                                             const int *__restrict__ labels, Geom g, int rpw, int nwaves,
                                                             RimRow *table) {
  rims_body<true>(w, dem, masks, labels, g, rpw, nwaves, table);
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
namespace {
inline unsigned blocks_for(long long items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }
}  // namespace

extern "C" int wdpm_rims_label(wdpm_ponds *h, double min_depth, int64_t *nponds) {
  if (!h) return wdpm_fail("wdpm_rims_label: null handle");
  if (!(min_depth >= 0.0) || std::isinf(min_depth)) return wdpm_fail("wdpm_rims_label: min_depth must be finite and >= 0 (got %g)", min_depth);
  if (h->seams) return wdpm_fail("wdpm_rims_label: the handle views a row block: rims are taken on whole rasters only");
  int64_t n = 0;
  if (wdpm_ponds_label(h, min_depth, &n)) return 1;           /* leaves masks, labels and the stream as the rim pass wants them */
  wdpm_ctx *x = h->x;
  const Geom g = h->g;
  const hipStream_t sm = x->stream;
  HIP_TRY(hipSetDevice(x->p.device));
  if (n > h->rims_cap) {                                      /* sized from N, like the pond table */
    guarded_free(h, h->d_rims);
    h->d_rims = nullptr;
    h->rims_cap = 0;
    const hipError_t e = guarded_malloc(h, (void **)&h->d_rims, (size_t)n * sizeof(RimRow));
    if (e != hipSuccess) return wdpm_fail("wdpm_rims_label: no device memory for the rims of %lld ponds: %s", (long long)n, hipGetErrorString(e));
    h->rims_cap = n;
  }
  h->rim_ms[0] = h->rim_ms[1] = 0.0;
  if (n > 0) {                                                /* no pond, no rim: nothing to launch */
    const size_t off = (size_t)h->row_off * g.ncp;
    const double *w = x->d_w[x->cur] + off, *dem = x->d_dem + off;
    const int rpw = ponds_rows_per_wave(g.nseg, g.rows, h->forced_rpw);
    const int nwaves = ((g.rows + rpw - 1) / rpw) * g.nsc;
    const unsigned nblocks = blocks_for(n, kBlock), wblocks = blocks_for(nwaves, kWaves);
    if (h->timing) HIP_TRY(hipEventRecord(h->rim_ev[0], sm));
    hipLaunchKernelGGL(rims_init_kernel, dim3(nblocks), dim3(kBlock), 0, sm, h->d_rims, (long long)n);
    hipLaunchKernelGGL(rims_pass_kernel, dim3(wblocks), dim3(kBlock), 0, sm, w, dem, h->d_masks, h->d_labels, g, rpw, nwaves, h->d_rims);
    if (h->timing) HIP_TRY(hipEventRecord(h->rim_ev[1], sm));
    hipLaunchKernelGGL(rims_locate_kernel, dim3(wblocks), dim3(kBlock), 0, sm, w, dem, h->d_masks, h->d_labels, g, rpw, nwaves, h->d_rims);
    hipLaunchKernelGGL(rims_finish_kernel, dim3(nblocks), dim3(kBlock), 0, sm, h->d_rims, (long long)n, g.ncp);
    if (h->timing) HIP_TRY(hipEventRecord(h->rim_ev[2], sm));
    HIP_TRY(hipGetLastError());
    if (wdpm_stream_sync(x, sm)) return 1;
    if (h->timing)
      for (int i = 0; i < WDPM_RIMS_PHASES; i++) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, h->rim_ev[i], h->rim_ev[i + 1]));
        h->rim_ms[i] = ms;
      }
  }
  h->rims_valid = true;
  if (nponds) *nponds = n;
  return 0;
}

extern "C" int wdpm_rims_table(wdpm_ponds *h, wdpm_pond_rim *out, int64_t capacity) {
  if (!h) return wdpm_fail("wdpm_rims_table: null handle");
  if (!h->valid || !h->rims_valid)
    return wdpm_fail("wdpm_rims_table: no rim table: the last label call on this handle was not a wdpm_rims_label that succeeded");
  const long long n = h->stats.ponds;
  if (capacity < n) return wdpm_fail("wdpm_rims_table: capacity %lld is too small for %lld ponds", (long long)capacity, n);
  if (n == 0) return 0;
  if (!out) return wdpm_fail("wdpm_rims_table: null output");
  if (wdpm_synchronize(h->x)) return 1;
  HIP_TRY(hipMemcpyAsync(out, h->d_rims, (size_t)n * sizeof(wdpm_pond_rim), hipMemcpyDeviceToHost, h->x->stream));
  return wdpm_stream_sync(h->x, h->x->stream);
}

extern "C" int wdpm_rims_phase_ms(wdpm_ponds *h, double *ms) {
  if (!h || !ms) return wdpm_fail("wdpm_rims_phase_ms: null argument");
  if (!h->timing) return wdpm_fail("wdpm_rims_phase_ms: the handle records no events (set WDPM_PONDS_TIMING=1 before it is made)");
  if (!h->valid || !h->rims_valid)
    return wdpm_fail("wdpm_rims_phase_ms: no rim table: the last label call on this handle was not a wdpm_rims_label that succeeded");
  for (int i = 0; i < WDPM_RIMS_PHASES; i++) ms[i] = h->rim_ms[i];
  return 0;
}
#endif  /* WDPM_PONDS_EMULATION */
