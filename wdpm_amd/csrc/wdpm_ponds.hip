/*
 * wdpm_ponds.hip — pond inventory (include/wdpm_ponds.h): label the 8-connected water bodies of a context's current raster on
 * the device, number them by first cell and accumulate one table row per pond.  gfx950.
 *
 * The unit stands beside the iteration library: it reads a context through wdpm_ctx.h like wdpm_rccl.hip does, owns every buffer
 * it writes, and none of its kernels is a launch of the iteration path (they are not in the launch ledger; tests/test_ponds.py
 * holds them against an independent host model instead).
 *
 * Work is done in RUNS, not cells.  A wave owns one 64-column segment of one row; __ballot of "is a pond cell" is the segment's
 * wet mask, and a run is a maximal string of set bits inside one segment, named by the padded cell index of its first cell.
 *
 *   mask     w, DEM -> wet masks (one uint64 per segment); every run start becomes its own parent
 *   merge    one union per pair of touching runs: run x run of the row above (8-connectivity: m & (up | up << 1 | up >> 1), with
 *            the edge bits of the neighbouring segments) and the run that continues over the segment's left seam.  Union-find on
 *            int32 parents; a link always points to a smaller index (atomicMin), so every chase ends and nobody waits for anybody
 *   flatten  every run start -> its root; per-segment root masks and counts
 *   scan     exclusive scan of the root counts in index order (three small kernels): the root of pond k is the k-th root
 *   table    labels for every cell; cells, volume_q, max depth and bounding box reduced per run, then per wave by label, then
 *            carried down the rows a wave owns, before one set of atomics per (wave, label change) goes to the table
 */
/* tests/ponds_emu_main.cpp compiles the kernels below for the host (256 threads per block in lockstep at the cross-lane operations,
 * address and undefined-behaviour sanitizers on) with WDPM_PONDS_EMULATION defined: tests/hip_emu.h brings the stand-ins for the HIP
 * device language and leaves the host half of this file out.  What this unit shares with wdpm_pond_rims.hip (geometry, depth keys,
 * wave helpers, the handle) lives in wdpm_ponds_priv.h. */
#include "wdpm_ponds_priv.h"
#ifndef WDPM_PONDS_EMULATION
#include "wdpm_ponds_stitch.h"
#endif

using namespace wdpm_pond_detail;   /* Geom, the depth keys, the table row and the handle's parts: shared with wdpm_pond_rims.hip */

namespace {

constexpr int kScanItems = 4;        /* segments per thread of the scan kernels */
constexpr int kScanTile = kBlock * kScanItems;
/* first bit of the run of `m` that holds bit `pos` (which is set) */
__device__ __forceinline__ int run_start(unsigned long long m, int pos) {
  const unsigned long long z = ~m & ((1ull << pos) - 1ull);
  return z ? 64 - __clzll((long long)z) : 0;
}
__device__ __forceinline__ int load_parent(const int *p, int x) {
  return __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int find_root(const int *p, int x) {
  for (;;) {
    const int q = load_parent(p, x);   /* q <= x always: the chase ends */
    if (q == x) return x;
    x = q;
  }
}
/* Lock-free union: link the larger root under the smaller.  atomicMin never raises a parent; when it replaced somebody else's
 * link (old != a), the pair (old, b) is still owed and the loop goes on with it - each retry follows a completed update. */
__device__ void unite(int *p, int a, int b) {
  for (;;) {
    a = find_root(p, a);
    b = find_root(p, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(p + a, b);
    if (old == a) return;
    a = old;
  }
}

/* ---- mask ------------------------------------------------------------------------------------------------------------------ */
__global__ __launch_bounds__(kBlock) void ponds_mask_kernel(const double *__restrict__ w, const double *__restrict__ dem, Geom g,
                                                            double min_depth, unsigned long long *__restrict__ masks,
                                                            int *__restrict__ parent, Status *st) {
  const int seg = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (seg >= g.nseg) return;
  const int lane = threadIdx.x & 63;
  const int r = seg / g.nsc, s = seg - r * g.nsc;
  const int c = s * kSeg + lane;
  bool wet = false;
  double depth = 0.0;
  int idx = 0;
  if (r >= 1 && r <= g.rows - 2 && c >= 1 && c <= g.ncp - 2) {
    idx = r * g.ncp + c;
    depth = w[idx];
    wet = dem[idx] < __builtin_inf() && depth > min_depth;
  }
  const unsigned long long m = __ballot(wet);
  if (lane == 0) masks[seg] = m;
  if (wet) {
    if (lane == 0 || !bit(m, lane - 1)) parent[idx] = idx;
    if (!(depth < 512.0)) st->deep = 1u;
  }
}

/* ---- merge ----------------------------------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(kBlock) void ponds_merge_kernel(const unsigned long long *__restrict__ masks, int *parent, Geom g,
                                                             unsigned *__restrict__ ucnt) {
  const int seg = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (seg >= g.nseg) return;
  const int lane = threadIdx.x & 63;
  const int r = seg / g.nsc, s = seg - r * g.nsc;
  const unsigned long long m = masks[seg];
  if (m == 0ull) { if (lane == 0) ucnt[seg] = 0u; return; }
  const bool above = r > 0;
  const unsigned long long up = above ? masks[seg - g.nsc] : 0ull;
  const unsigned long long upl = (above && s > 0) ? masks[seg - g.nsc - 1] : 0ull;
  const unsigned long long upr = (above && s < g.nsc - 1) ? masks[seg - g.nsc + 1] : 0ull;
  const unsigned long long left = s > 0 ? masks[seg - 1] : 0ull;

  const bool wet = bit(m, lane);
  const int row_base = r * g.ncp + s * kSeg, up_base = row_base - g.ncp;
  const int up_c = bit(up, lane);
  const int up_m = lane > 0 ? bit(up, lane - 1) : bit(upl, 63);
  const int up_p = lane < 63 ? bit(up, lane + 1) : bit(upr, 0);
  const bool start = wet && (lane == 0 || !bit(m, lane - 1));
  const int me = row_base + run_start(m, lane);

  /* A: a run start meets the run above that covers its column or the one before it */
  const bool a_do = start && (up_c || up_m);
  const bool a_seam = a_do && !up_c && lane == 0;
  /* B: a run of the row above that begins one column further right is first met by this cell */
  const bool b_do = wet && up_p && !up_c;
  const bool b_seam = b_do && lane == 63;
  /* C: the run goes on over the segment's left seam */
  const bool c_do = wet && lane == 0 && bit(left, 63);

  if (a_do) {
    int other;
    if (up_c) other = up_base + run_start(up, lane);
    else if (lane > 0) other = up_base + run_start(up, lane - 1);
    else other = up_base - kSeg + run_start(upl, 63);
    unite(parent, me, other);
  }
  if (b_do) unite(parent, me, up_base + lane + 1);
  if (c_do) unite(parent, me, row_base - kSeg + run_start(left, 63));

  const unsigned n_all = __popcll(__ballot(a_do)) + __popcll(__ballot(b_do)) + __popcll(__ballot(c_do));
  const unsigned n_seam = __popcll(__ballot(a_seam)) + __popcll(__ballot(b_seam)) + __popcll(__ballot(c_do));
  if (lane == 0) ucnt[seg] = n_all | (n_seam << 16);   /* at most 129 and 3 */
}

/* ---- flatten --------------------------------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(kBlock) void ponds_flatten_kernel(const unsigned long long *__restrict__ masks, int *parent, Geom g,
                                                               int *__restrict__ cnt, unsigned long long *__restrict__ rootmask) {
  const int seg = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (seg >= g.nseg) return;
  const int lane = threadIdx.x & 63;
  const int r = seg / g.nsc, s = seg - r * g.nsc;
  const unsigned long long m = masks[seg];
  bool is_root = false;
  if (bit(m, lane) && (lane == 0 || !bit(m, lane - 1))) {
    const int idx = r * g.ncp + s * kSeg + lane;
    const int root = find_root(parent, idx);
    /* readers in flight see the old parent or the root: both are ancestors */
    __hip_atomic_store(parent + idx, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    is_root = root == idx;
  }
  const unsigned long long rm = __ballot(is_root);
  if (lane == 0) { cnt[seg] = __popcll(rm); rootmask[seg] = rm; }
}

/* ---- scan of the root counts ------------------------------------------------------------------------------------------------ */
/* exclusive scan of one int per thread over the block; total = the block's sum */
__device__ __forceinline__ int block_exclusive_scan(int v, int &total, int *lds /* kWaves + 1 ints */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(inc, d);
    if (lane >= d) inc += t;
  }
  __syncthreads();                 /* lds may still be read from the previous call */
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  int off = 0, sum = 0;
#pragma unroll
  for (int i = 0; i < kWaves; i++) {
    if (i < wave) off += lds[i];
    sum += lds[i];
  }
  total = sum;
  return off + inc - v;
}

__global__ __launch_bounds__(kBlock) void ponds_scan_reduce_kernel(const int *__restrict__ cnt, const unsigned *__restrict__ ucnt,
                                                                   int nseg, int *__restrict__ bsum,
                                                                   unsigned long long *__restrict__ busum) {
  __shared__ int lds[kWaves + 1];
  __shared__ unsigned long long ulds[2 * kWaves];
  const int i0 = blockIdx.x * kScanTile + threadIdx.x * kScanItems;
  int v = 0;
  unsigned long long un = 0ull, us = 0ull;
#pragma unroll
  for (int k = 0; k < kScanItems; k++)
    if (i0 + k < nseg) {
      v += cnt[i0 + k];
      const unsigned u = ucnt[i0 + k];
      un += u & 0xffffu;
      us += u >> 16;
    }
  int total;
  (void)block_exclusive_scan(v, total, lds);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    un += __shfl_xor(un, d);
    us += __shfl_xor(us, d);
  }
  if ((threadIdx.x & 63) == 0) { ulds[threadIdx.x >> 6] = un; ulds[kWaves + (threadIdx.x >> 6)] = us; }
  __syncthreads();
  if (threadIdx.x == 0) {
    bsum[blockIdx.x] = total;
    unsigned long long a = 0ull, b = 0ull;
    for (int i = 0; i < kWaves; i++) { a += ulds[i]; b += ulds[kWaves + i]; }
    busum[2 * blockIdx.x] = a;
    busum[2 * blockIdx.x + 1] = b;
  }
}

/* one block: block sums -> their exclusive scan in place, the totals into the status words */
__global__ __launch_bounds__(kBlock) void ponds_scan_sums_kernel(int *bsum, const unsigned long long *__restrict__ busum, int nb,
                                                                 Status *st) {
  __shared__ int lds[kWaves + 1];
  __shared__ unsigned long long ulds[2 * kWaves];
  long long carry = 0;
  unsigned long long un = 0ull, us = 0ull;
  for (int base = 0; base < nb; base += kBlock) {
    const int i = base + threadIdx.x;
    const int v = i < nb ? bsum[i] : 0;
    if (i < nb) { un += busum[2 * i]; us += busum[2 * i + 1]; }
    int total;
    const int ex = block_exclusive_scan(v, total, lds);
    if (i < nb) bsum[i] = (int)(carry + ex);
    carry += total;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    un += __shfl_xor(un, d);
    us += __shfl_xor(us, d);
  }
  if ((threadIdx.x & 63) == 0) { ulds[threadIdx.x >> 6] = un; ulds[kWaves + (threadIdx.x >> 6)] = us; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long a = 0ull, b = 0ull;
    for (int i = 0; i < kWaves; i++) { a += ulds[i]; b += ulds[kWaves + i]; }
    st->ponds = carry;
    st->unions = a;
    st->seam_unions = b;
  }
}

/* per-segment root counts -> the number of roots before the segment, in place */
__global__ __launch_bounds__(kBlock) void ponds_scan_down_kernel(int *cnt, int nseg, const int *__restrict__ bsum) {
  __shared__ int lds[kWaves + 1];
  const int i0 = blockIdx.x * kScanTile + threadIdx.x * kScanItems;
  int c[kScanItems], v = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; k++) {
    c[k] = i0 + k < nseg ? cnt[i0 + k] : 0;
    v += c[k];
  }
  int total;
  int run = bsum[blockIdx.x] + block_exclusive_scan(v, total, lds);
#pragma unroll
  for (int k = 0; k < kScanItems; k++) {
    if (i0 + k < nseg) cnt[i0 + k] = run;
    run += c[k];
  }
}

/* ---- table ----------------------------------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(kBlock) void ponds_table_init_kernel(PondRow *t, long long n) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  PondRow r;
  r.first_row = r.first_col = 0;
  r.cells = 0ull; r.volume_q = 0ull; r.depth_key = 0ull;
  r.row_min = r.col_min = INT_MAX;
  r.row_max = r.col_max = -1;
  t[i] = r;
}

__global__ __launch_bounds__(kBlock) void ponds_table_finish_kernel(PondRow *t, long long n) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const double d = depth_from_key(t[i].depth_key);
  t[i].depth_key = (unsigned long long)__double_as_longlong(d);
}

/* what a wave has gathered for one label and not yet sent */
struct Carry {
  int label;               /* 0: nothing held */
  unsigned long long cells, vol, key;
  int row_min, row_max, col_min, col_max;
};

/* one lane sends a carry: the extrema through atomic_min_if / atomic_max_if */
__device__ __forceinline__ void send(PondRow *table, const Carry &c) {
  PondRow *t = table + (c.label - 1);
  atomicAdd(&t->cells, c.cells);
  atomicAdd(&t->volume_q, c.vol);
  atomic_max_if(&t->depth_key, c.key);
  atomic_min_if(&t->row_min, c.row_min);
  atomic_max_if(&t->row_max, c.row_max);
  atomic_min_if(&t->col_min, c.col_min);
  atomic_max_if(&t->col_max, c.col_max);
}

/* the label of the run that starts at cell idx: its root's rank among the roots, from 1 */
__device__ __forceinline__ int label_of_run(const int *__restrict__ parent, const int *__restrict__ base,
                                            const unsigned long long *__restrict__ rootmask, const Geom &g, int idx, int &root) {
  root = parent[idx];
  const int rr = root / g.ncp, rc = root - rr * g.ncp;
  const int rseg = rr * g.nsc + rc / kSeg, rbit = rc % kSeg;
  return base[rseg] + __popcll(rootmask[rseg] & ((1ull << rbit) - 1ull)) + 1;
}

/* A wave owns segment column s of rows [r0, r0 + rpw).  Everything that steers the loops below is wave-uniform.
 * kMapped (row blocks): the label raster takes map[label - 1], the pond's number in the whole raster, looked up once per run
 * where its label is computed; the table stays indexed by the label itself. */
template <bool kMapped>
__device__ __forceinline__ void ponds_table_body(const double *__restrict__ w, const unsigned long long *__restrict__ masks,
                                                 const int *__restrict__ parent, const int *__restrict__ base,
                                                 const unsigned long long *__restrict__ rootmask, const Geom g, const int rpw,
                                                 const int nwaves, int *__restrict__ labels, PondRow *table,
                                                 const int *__restrict__ map) {
  const int wid = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (wid >= nwaves) return;
  const int lane = threadIdx.x & 63;
  const int rb = wid / g.nsc, s = wid - rb * g.nsc;
  const int r0 = rb * rpw, r1 = min(r0 + rpw, g.rows);
  const int c = s * kSeg + lane;
  const bool inside = c < g.ncp;
  Carry cy;
  cy.label = 0; cy.cells = cy.vol = cy.key = 0ull;
  cy.row_min = cy.col_min = INT_MAX; cy.row_max = cy.col_max = -1;

  for (int r = r0; r < r1; r++) {
    const unsigned long long m = masks[r * g.nsc + s];
    const int idx = r * g.ncp + c;
    if (m == 0ull) {
      if (inside) labels[idx] = 0;
      continue;
    }
    const bool wet = bit(m, lane);
    const int st = wet ? run_start(m, lane) : lane;
    int label = 0, shown = 0;
    if (wet && st == lane) {               /* a run start: where is its root among the roots? */
      int root;
      label = label_of_run(parent, base, rootmask, g, idx, root);
      if (root == idx) { table[label - 1].first_row = r; table[label - 1].first_col = c; }
      if (kMapped) shown = map[label - 1];
    }
    label = __shfl(label, st);
    if (!wet) label = 0;
    if (kMapped) {
      shown = __shfl(shown, st);
      if (!wet) shown = 0;
    } else {
      shown = label;
    }
    if (inside) labels[idx] = shown;

    /* per run: a segmented scan leaves each run's sum and maximum in its last lane */
    unsigned long long q = 0ull, k = 0ull;
    if (wet) {
      const double d = w[idx];
      q = (unsigned long long)rint(d * 16777216.0);
      k = depth_key(d);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long tq = __shfl_up(q, d), tk = __shfl_up(k, d);
      if (wet && lane - d >= st) { q += tq; k = tk > k ? tk : k; }
    }
    const unsigned long long lastm = m & ~(m >> 1);
    /* per wave, by label: the runs of one label are gathered from their last lanes */
    unsigned long long pending = lastm;
    while (pending) {
      const int l0 = __builtin_ctzll(pending);
      const int L = __shfl(label, l0);
      const unsigned long long cellm = __ballot(wet && label == L);
      const unsigned long long match = cellm & lastm;
      unsigned long long vs = 0ull, vk = 0ull;
      for (unsigned long long t = match; t; t &= t - 1ull) {
        const int b = __builtin_ctzll(t);
        vs += __shfl(q, b);
        const unsigned long long tk = __shfl(k, b);
        vk = tk > vk ? tk : vk;
      }
      pending &= ~match;
      const int cmin = s * kSeg + __builtin_ctzll(cellm), cmax = s * kSeg + 63 - __clzll((long long)cellm);
      if (cy.label != L) {                  /* down the rows: the same label goes on gathering, another one sends first */
        if (cy.label != 0 && lane == 0) send(table, cy);
        cy.label = L; cy.cells = cy.vol = cy.key = 0ull;
        cy.row_min = r; cy.col_min = INT_MAX; cy.row_max = cy.col_max = -1;
      }
      cy.cells += (unsigned long long)__popcll(cellm);
      cy.vol += vs;
      cy.key = vk > cy.key ? vk : cy.key;
      cy.row_max = r;
      cy.col_min = min(cy.col_min, cmin);
      cy.col_max = max(cy.col_max, cmax);
    }
  }
  if (cy.label != 0 && lane == 0) send(table, cy);
}

__global__ __launch_bounds__(kBlock) void ponds_table_kernel(const double *__restrict__ w, const unsigned long long *__restrict__ masks,
                                                             const int *__restrict__ parent, const int *__restrict__ base,
                                                             const unsigned long long *__restrict__ rootmask, Geom g, int rpw,
                                                             int nwaves, int *__restrict__ labels, PondRow *table) {
  ponds_table_body<false>(w, masks, parent, base, rootmask, g, rpw, nwaves, labels, table, nullptr);
}

__global__ __launch_bounds__(kBlock) void ponds_table_mapped_kernel(const double *__restrict__ w, const unsigned long long *__restrict__ masks,
                                                                    const int *__restrict__ parent, const int *__restrict__ base,
                                                                    const unsigned long long *__restrict__ rootmask, Geom g, int rpw,
                                                                    int nwaves, int *__restrict__ labels, PondRow *table,
                                                                    const int *__restrict__ map) {
  ponds_table_body<true>(w, masks, parent, base, rootmask, g, rpw, nwaves, labels, table, map);
}

/* ---- seam rows (row blocks) -------------------------------------------------------------------------------------------------- */
/* After the scan: the labels of the view's first and last inner row (rows 1 and g.rows - 2), g.ncp int32 each, for the host
 * that joins neighbouring row blocks.  One wave per segment of either row. */
__global__ __launch_bounds__(kBlock) void ponds_seam_kernel(const unsigned long long *__restrict__ masks, const int *__restrict__ parent,
                                                            const int *__restrict__ base, const unsigned long long *__restrict__ rootmask,
                                                            Geom g, int *__restrict__ seam) {
  const int wid = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (wid >= 2 * g.nsc) return;
  const int lane = threadIdx.x & 63;
  const int side = wid / g.nsc, s = wid - side * g.nsc;
  const int r = side ? g.rows - 2 : 1;
  const int c = s * kSeg + lane;
  const unsigned long long m = masks[r * g.nsc + s];
  const bool wet = bit(m, lane);
  const int st = wet ? run_start(m, lane) : lane;
  int label = 0;
  if (wet && st == lane) {
    int root;
    label = label_of_run(parent, base, rootmask, g, r * g.ncp + c, root);
  }
  label = __shfl(label, st);
  if (!wet) label = 0;
  if (c < g.ncp) seam[side * g.ncp + c] = label;
}

}  // namespace

#ifndef WDPM_PONDS_EMULATION
/* ---- host ------------------------------------------------------------------------------------------------------------------ */
namespace wdpm_pond_detail {

hipError_t guarded_malloc(wdpm_ponds *h, void **p, size_t bytes) {
  char *base = nullptr;
  hipError_t e = hipMalloc(&base, bytes + 2 * h->guard);
  if (e != hipSuccess) return e;
  if (h->guard) {
    e = hipMemset(base, 0xA5, h->guard);
    if (e == hipSuccess) e = hipMemset(base + h->guard + bytes, 0xA5, h->guard);
    if (e != hipSuccess) { (void)hipFree(base); return e; }
    h->guards.push_back({base, bytes});
  }
  *p = base + h->guard;
  return hipSuccess;
}

void guarded_free(wdpm_ponds *h, void *p) {
  if (!p) return;
  char *base = static_cast<char *>(p) - h->guard;
  for (size_t i = 0; i < h->guards.size(); i++)
    if (h->guards[i].base == base) { h->guards.erase(h->guards.begin() + i); break; }
  (void)hipFree(base);
}

}  // namespace wdpm_pond_detail

namespace {

/* gives every buffer back and leaves the handle as it was made: one line per holder */
void release(wdpm_ponds *h) {
  LabelUnit &l = h->lab;
  reset(h, l.masks); reset(h, l.rootmask); reset(h, l.busum); reset(h, l.parent); reset(h, l.labels); reset(h, l.cnt); reset(h, l.bsum);
  reset(h, l.ucnt); reset(h, l.status); reset(h, l.seam); reset(h, l.h_seam); reset(h, l.map); reset(h, l.h_map); reset(h, l.h_table);
  reset(h, l.table);
  reset(h, h->rim.table); reset(h, h->rim.slot_of); reset(h, h->rim.foreign); reset(h, h->rim.h_beside); reset(h, h->rim.h_table);
  reset(h, h->cat.link); reset(h, h->cat.table); reset(h, h->cat.status); reset(h, h->cat.keys); reset(h, h->cat.h_keys);
  reset(h, h->cat.exits); reset(h, h->cat.h_exits); reset(h, h->cat.h_table);
  reset(h, h->out.table); reset(h, h->out.status); reset(h, h->out.keys); reset(h, h->out.h_keys); reset(h, h->out.h_table);
  reset(h, h->out.h_seam);
  reset(h, h->cur.table); reset(h, h->cur.status); reset(h, h->cur.keys); reset(h, h->cur.h_keys); reset(h, h->cur.h_table);
  reset(h, h->spl.table); reset(h, h->spl.words); reset(h, h->spl.sums); reset(h, h->spl.status);
  reset(h, h->rte.table); reset(h, h->rte.words); reset(h, h->rte.sums); reset(h, h->rte.status); reset(h, h->rte.h_offsets);
  l.allocated = l.valid = h->rim.valid = h->cat.valid = h->out.valid = h->cur.valid = h->spl.valid = h->rte.valid = false;
}

int allocate(wdpm_ponds *h) {
  LabelUnit &l = h->lab;
  if (l.allocated) return 0;
  const long long cells = (long long)h->g.rows * h->g.ncp, nseg = h->g.nseg;
  l.nb = (int)((nseg + kScanTile - 1) / kScanTile);
  const char *what;
  hipError_t e = grow(h, l.masks, nseg);
  if (e == hipSuccess) e = grow(h, l.rootmask, nseg);
  if (e == hipSuccess) e = grow(h, l.parent, cells);
  if (e == hipSuccess) e = grow(h, l.labels, cells);
  if (e == hipSuccess) e = grow(h, l.cnt, nseg);
  if (e == hipSuccess) e = grow(h, l.ucnt, nseg);
  if (e == hipSuccess) e = grow(h, l.bsum, l.nb);
  if (e == hipSuccess) e = grow(h, l.busum, 2LL * l.nb);
  if (e == hipSuccess) e = ensure(l.status, &what);
  if (h->seams) {
    if (e == hipSuccess) e = grow(h, l.seam, 2LL * h->g.ncp);
    if (e == hipSuccess) e = grow(h, l.h_seam, 2LL * h->g.ncp);
  }
  if (e != hipSuccess) {
    release(h);                     /* what was taken so far: the next call starts from nothing again */
    return wdpm_fail("wdpm_ponds_label: device allocation failed: %s", hipGetErrorString(e));
  }
  l.allocated = true;
  return 0;
}

/* a handle on rows [row_off, row_off + rows) of ctx; reads the environment as include/wdpm_ponds.h says */
wdpm_ponds *make_handle(wdpm_ctx *ctx, int row_off, int rows, bool seams) {
  wdpm_ponds *h = new wdpm_ponds();
  h->x = ctx;
  h->row_off = row_off;
  h->seams = seams;
  h->g.rows = rows;
  h->g.ncp = ctx->g.ncp;
  h->g.nsc = (ctx->g.ncp + kSeg - 1) / kSeg;
  h->g.nseg = h->g.rows * h->g.nsc;             /* <= cells / 64 + rows: an int with 2^31 - 1 cells */
  const char *e = getenv("WDPM_GUARD_KB");
  const long kb = e ? atol(e) : 0;
  h->guard = kb > 0 ? (size_t)kb * 1024 : 0;
  { const char *re = getenv("WDPM_PONDS_ROWS_PER_WAVE"); h->forced_rpw = re ? atoi(re) : 0; }
  const char *te = getenv("WDPM_PONDS_TIMING");
  h->timing = te && atoi(te) != 0;
  h->lab.timer.create(h->timing);
  h->rim.timer.create(h->timing);
  h->cat.timer.create(h->timing);
  h->out.timer.create(h->timing);
  h->cur.timer.create(h->timing);
  h->spl.timer.create(h->timing);
  h->rte.timer.create(h->timing);
  h->rte.narrow = route_bound(getenv("WDPM_ROUTE_NARROW"), 1, kBlock, kBlock);
  h->rte.run_levels = route_bound(getenv("WDPM_ROUTE_RUN_LEVELS"), 1, INT_MAX, kRouteRunLevels);
  return h;
}

/* ---- a label call in four steps: the two that queue work never wait for it, so a group queues every rank before it waits for
 * the first.  wdpm_ponds_label runs them back to back. ---- */

/* 1: mask, merge, flatten, scan (and the seam rows of a row block), status words on their way to the host */
int label_queue(wdpm_ponds *h, double min_depth) {
  wdpm_ctx *x = h->x;
  h->lab.valid = false;
  h->rim.valid = false;             /* a rim table belongs to the label call that made it (wdpm_pond_rims.hip) */
  h->cat.valid = false;             /* and so does a catchment table (wdpm_pond_catchments.hip) */
  h->out.valid = false;             /* and an outlet table (wdpm_pond_outlets.hip) */
  h->cur.valid = false;             /* and a curve table (wdpm_pond_curves.hip) */
  h->spl.valid = false;             /* and a spill table (wdpm_pond_spills.hip) */
  h->rte.valid = false;             /* and a routing table (wdpm_pond_routing.hip) */
  /* the raster as a reader sees it: side stream joined, owed drain() and threshold flush applied (what wdpm_count_stats asks for) */
  if (wdpm_synchronize(x)) return 1;
  if (wdpm_apply_owed_flush(x)) return 1;
  if (allocate(h)) return 1;
  const Geom g = h->g;
  const hipStream_t sm = x->stream;
  const size_t off = (size_t)h->row_off * g.ncp;
  const double *w = x->d_w[x->cur] + off;
  const unsigned seg_blocks = blocks_for(g.nseg, kWaves);

  HIP_TRY(hipMemsetAsync(h->lab.status.d, 0, sizeof(Status), sm));
  HIP_TRY(h->lab.timer.mark(h->timing, 0, sm));
  hipLaunchKernelGGL(ponds_mask_kernel, dim3(seg_blocks), dim3(kBlock), 0, sm, w, x->d_dem + off, g, min_depth, h->lab.masks.p, h->lab.parent.p, h->lab.status.d);
  HIP_TRY(h->lab.timer.mark(h->timing, 1, sm));
  hipLaunchKernelGGL(ponds_merge_kernel, dim3(seg_blocks), dim3(kBlock), 0, sm, h->lab.masks.p, h->lab.parent.p, g, h->lab.ucnt.p);
  HIP_TRY(h->lab.timer.mark(h->timing, 2, sm));
  hipLaunchKernelGGL(ponds_flatten_kernel, dim3(seg_blocks), dim3(kBlock), 0, sm, h->lab.masks.p, h->lab.parent.p, g, h->lab.cnt.p, h->lab.rootmask.p);
  HIP_TRY(h->lab.timer.mark(h->timing, 3, sm));
  hipLaunchKernelGGL(ponds_scan_reduce_kernel, dim3(h->lab.nb), dim3(kBlock), 0, sm, h->lab.cnt.p, h->lab.ucnt.p, g.nseg, h->lab.bsum.p, h->lab.busum.p);
  hipLaunchKernelGGL(ponds_scan_sums_kernel, dim3(1), dim3(kBlock), 0, sm, h->lab.bsum.p, h->lab.busum.p, h->lab.nb, h->lab.status.d);
  hipLaunchKernelGGL(ponds_scan_down_kernel, dim3(h->lab.nb), dim3(kBlock), 0, sm, h->lab.cnt.p, g.nseg, h->lab.bsum.p);
  if (h->seams)
    hipLaunchKernelGGL(ponds_seam_kernel, dim3(blocks_for(2 * g.nsc, kWaves)), dim3(kBlock), 0, sm, h->lab.masks.p, h->lab.parent.p, h->lab.cnt.p,
                       h->lab.rootmask.p, g, h->lab.seam.p);
  HIP_TRY(h->lab.timer.mark(h->timing, 4, sm));
  HIP_TRY(hipGetLastError());
  if (h->seams) HIP_TRY(hipMemcpyAsync(h->lab.h_seam.p, h->lab.seam.p, (size_t)2 * g.ncp * sizeof(int), hipMemcpyDeviceToHost, sm));
  HIP_TRY(hipMemcpyAsync(h->lab.status.h, h->lab.status.d, sizeof(Status), hipMemcpyDeviceToHost, sm));
  return 0;
}

/* 2: wait for 1; N of the view */
int label_status(wdpm_ponds *h, long long *n) {
  HIP_TRY(hipSetDevice(h->x->p.device));
  if (wdpm_stream_sync(h->x, h->x->stream)) return 1;
  h->lab.last = *h->lab.status.h;
  if (h->lab.last.deep)
    return wdpm_fail("wdpm_ponds_label: a pond cell holds 512 m of water or more: volume_q (a 64-bit sum of depths in units of "
                     "2^-24 m) is only safe below that depth");
  *n = h->lab.last.ponds;
  return 0;
}

/* 3: the table kernels.  With `mapped` (row blocks; `map` holds n ints, copied here) the label raster takes map[label - 1] and the
 * finished table follows to h->lab.h_table.p.  Map and table travel through pinned memory, so every transfer is queued like the
 * kernels and the call returns without waiting for any of them; the pinned buffers grow only when N outgrows them. */
int table_queue(wdpm_ponds *h, bool mapped, const int *map) {
  wdpm_ctx *x = h->x;
  const Geom g = h->g;
  const hipStream_t sm = x->stream;
  const long long n = h->lab.last.ponds;
  const double *w = x->d_w[x->cur] + (size_t)h->row_off * g.ncp;
  HIP_TRY(hipSetDevice(x->p.device));
  hipError_t e = grow(h, h->lab.table, n);      /* sized from N, now that N is known */
  if (e != hipSuccess) return wdpm_fail("wdpm_ponds_label: no device memory for a table of %lld ponds: %s", n, hipGetErrorString(e));
  if (mapped) {
    e = grow(h, h->lab.map, n);
    if (e != hipSuccess) return wdpm_fail("wdpm_group_ponds_label: no device memory for the numbers of %lld ponds: %s", n, hipGetErrorString(e));
    if (n > h->lab.h_map.cap) { reset(h, h->lab.h_map); reset(h, h->lab.h_table); }   /* the two grow together: both go before either comes */
    e = grow(h, h->lab.h_map, n);
    if (e == hipSuccess) e = grow(h, h->lab.h_table, n);
    if (e != hipSuccess) return wdpm_fail("wdpm_group_ponds_label: no pinned host memory for %lld ponds: %s", n, hipGetErrorString(e));
  }
  if (mapped && n > 0) {
    memcpy(h->lab.h_map.p, map, (size_t)n * sizeof(int));
    HIP_TRY(hipMemcpyAsync(h->lab.map.p, h->lab.h_map.p, (size_t)n * sizeof(int), hipMemcpyHostToDevice, sm));
  }
  const Waves wv = waves_for(h, g.rows);
  const int rpw = h->lab.rpw = wv.rpw, nwaves = wv.nwaves;
  HIP_TRY(h->lab.timer.mark(h->timing, 5, sm));
  if (n > 0) hipLaunchKernelGGL(ponds_table_init_kernel, dim3(blocks_for(n, kBlock)), dim3(kBlock), 0, sm, h->lab.table.p, n);
  if (mapped)
    hipLaunchKernelGGL(ponds_table_mapped_kernel, dim3(blocks_for(nwaves, kWaves)), dim3(kBlock), 0, sm, w, h->lab.masks.p, h->lab.parent.p,
                       h->lab.cnt.p, h->lab.rootmask.p, g, rpw, nwaves, h->lab.labels.p, h->lab.table.p, h->lab.map.p);
  else
    hipLaunchKernelGGL(ponds_table_kernel, dim3(blocks_for(nwaves, kWaves)), dim3(kBlock), 0, sm, w, h->lab.masks.p, h->lab.parent.p, h->lab.cnt.p,
                       h->lab.rootmask.p, g, rpw, nwaves, h->lab.labels.p, h->lab.table.p);
  HIP_TRY(h->lab.timer.mark(h->timing, 6, sm));
  if (n > 0) hipLaunchKernelGGL(ponds_table_finish_kernel, dim3(blocks_for(n, kBlock)), dim3(kBlock), 0, sm, h->lab.table.p, n);
  HIP_TRY(h->lab.timer.mark(h->timing, 7, sm));
  HIP_TRY(hipGetLastError());
  if (mapped && n > 0) HIP_TRY(hipMemcpyAsync(h->lab.h_table.p, h->lab.table.p, (size_t)n * sizeof(wdpm_pond), hipMemcpyDeviceToHost, sm));
  return 0;
}

/* 4: wait for 3; the handle has an inventory */
int table_wait(wdpm_ponds *h) {
  HIP_TRY(hipSetDevice(h->x->p.device));
  if (wdpm_stream_sync(h->x, h->x->stream)) return 1;
  if (h->timing) {
    /* mask, merge, flatten, scan, (host: status, table allocation), table init + table, finish */
    static const int from[WDPM_PONDS_PHASES] = {0, 1, 2, 3, 5, 6}, to[WDPM_PONDS_PHASES] = {1, 2, 3, 4, 6, 7};
    for (int i = 0; i < WDPM_PONDS_PHASES; i++) HIP_TRY(h->lab.timer.read(from[i], to[i], &h->lab.timer.ms[i]));
  }
  h->lab.stats.segments = h->g.nseg;
  h->lab.stats.unions = (int64_t)h->lab.last.unions;
  h->lab.stats.seam_unions = (int64_t)h->lab.last.seam_unions;
  h->lab.stats.passes = 0;
  h->lab.stats.rows_per_wave = h->lab.rpw;
  h->lab.stats.ponds = h->lab.last.ponds;
  h->lab.valid = true;
  return 0;
}

int count_guard_bad(wdpm_ponds *h, int64_t *bytes) {
  if (!h->guard || h->guards.empty()) return 0;
  if (wdpm_synchronize(h->x)) return 1;
  std::vector<unsigned char> buf(h->guard);
  for (const Guarded &gb : h->guards)
    for (int side = 0; side < 2; side++) {
      HIP_TRY(hipMemcpy(buf.data(), gb.base + (side ? h->guard + gb.bytes : 0), h->guard, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < h->guard; i++) *bytes += buf[i] != 0xA5;
    }
  return 0;
}

void destroy_handle(wdpm_ponds *h) {
  if (!h) return;
  (void)wdpm_synchronize(h->x);
  release(h);
  h->lab.timer.destroy();
  h->rim.timer.destroy();
  h->cat.timer.destroy();
  h->out.timer.destroy();
  h->cur.timer.destroy();
  h->spl.timer.destroy();
  h->rte.timer.destroy();
  delete h;
}

const char kNoTable[] = "no inventory: wdpm_ponds_label has not succeeded on this handle";
const char kNoGroupTable[] = "no inventory: wdpm_group_ponds_label has not succeeded on this handle";

}  // namespace

extern "C" int wdpm_ponds_create(wdpm_ponds **out, wdpm_ctx *ctx) {
  if (!out || !ctx) return wdpm_fail("wdpm_ponds_create: null argument");
  const SlabGeom &sg = ctx->g;
  if (sg.row0 != 0 || sg.rows != sg.R + 2)
    return wdpm_fail("wdpm_ponds_create: a slab context (rows %d..%d of %d) cannot take an inventory: ponds cross row blocks; "
                     "use a context that holds the whole raster", sg.row0, sg.row0 + sg.rows, sg.R + 2);
  if (wdpm_synchronize(ctx)) return 1;          /* binds the device */
  *out = make_handle(ctx, 0, sg.rows, false);
  return 0;
}

extern "C" void wdpm_ponds_destroy(wdpm_ponds *h) { destroy_handle(h); }

extern "C" int wdpm_ponds_label(wdpm_ponds *h, double min_depth, int64_t *nponds) {
  if (!h) return wdpm_fail("wdpm_ponds_label: null handle");
  if (check_min_depth("wdpm_ponds_label", min_depth)) return 1;
  long long n = 0;
  if (label_queue(h, min_depth) || label_status(h, &n) || table_queue(h, false, nullptr) || table_wait(h)) return 1;
  if (nponds) *nponds = n;
  return 0;
}

extern "C" int wdpm_ponds_table(wdpm_ponds *h, wdpm_pond *out, int64_t capacity) {
  return table_out("wdpm_ponds_table", h, &wdpm_ponds::lab, kNoTable, out, capacity);
}

extern "C" int wdpm_ponds_labels(wdpm_ponds *h, int32_t *padded) {
  if (!h || !padded) return wdpm_fail("wdpm_ponds_labels: null argument");
  if (!h->lab.valid) return wdpm_fail("wdpm_ponds_labels: %s", kNoTable);
  return download(h, padded, h->lab.labels.p, (size_t)h->g.rows * h->g.ncp * sizeof(int32_t));
}

extern "C" int wdpm_ponds_guard_bad(wdpm_ponds *h, int64_t *bytes) {
  if (!h || !bytes) return wdpm_fail("wdpm_ponds_guard_bad: null argument");
  *bytes = 0;
  return count_guard_bad(h, bytes);
}

extern "C" int wdpm_ponds_stats(wdpm_ponds *h, wdpm_pond_stats *out) {
  return stats_out("wdpm_ponds_stats", h, &wdpm_ponds::lab, kNoTable, out, true);
}

extern "C" int wdpm_ponds_phase_ms(wdpm_ponds *h, double *ms) {
  return phase_ms_out("wdpm_ponds_phase_ms", h, &wdpm_ponds::lab, kNoTable, ms, true);
}

/* ---- row blocks (include/wdpm_group_ponds.h) --------------------------------------------------------------------------------- */
/* (struct wdpm_group_ponds: wdpm_ponds_priv.h) */
extern "C" int wdpm_group_ponds_create(wdpm_group_ponds **out, wdpm_group *grp) {
  if (!out || !grp) return wdpm_fail("wdpm_group_ponds_create: null argument");
  const int n = wdpm_group_size(grp);
  if (n < 1) return wdpm_fail("wdpm_group_ponds_create: the group has no rank");
  wdpm_group_ponds *h = new wdpm_group_ponds();
  h->grp = grp;
  h->n = n;
  for (int i = 0; i < n; i++) {
    wdpm_rank *rk = wdpm_group_rank(grp, i);
    wdpm_ctx *x = rk ? wdpm_rank_ctx(rk) : nullptr;
    wdpm_slab s;
    if (!x || (n > 1 && wdpm_rank_slab(rk, -1, &s))) {
      wdpm_group_ponds_destroy(h);
      return wdpm_fail("wdpm_group_ponds_create: rank %d of the group cannot be read", i);
    }
    const int P = x->g.R + 2;
    if (n == 1) { s.own_lo = 0; s.own_hi = P - 1; s.row0 = 0; }
    /* owned rows and one row either side (the halos hold them); the raster's own border row at either end */
    const int v0 = s.own_lo > 0 ? s.own_lo - 1 : 0, v1 = s.own_hi < P - 1 ? s.own_hi + 1 : P - 1;
    if (v0 < x->g.row0 || v1 >= x->g.row0 + x->g.rows || v1 - v0 + 1 < 3) {
      wdpm_group_ponds_destroy(h);
      return wdpm_fail("wdpm_group_ponds_create: rank %d holds rows %d..%d, its owned rows %d..%d want one more either side", i,
                       x->g.row0, x->g.row0 + x->g.rows - 1, s.own_lo, s.own_hi);
    }
    if ((long long)(v1 - v0 + 1) * x->g.ncp > (long long)INT_MAX) {
      wdpm_group_ponds_destroy(h);
      return wdpm_fail("wdpm_group_ponds_create: rank %d would label %lld cells, more than 2^31 - 1: use more row blocks", i,
                       (long long)(v1 - v0 + 1) * x->g.ncp);
    }
    if (wdpm_synchronize(x)) { wdpm_group_ponds_destroy(h); return 1; }   /* binds the device */
    wdpm_ponds *p = make_handle(x, v0 - x->g.row0, v1 - v0 + 1, true);
    h->r.push_back(p);
    h->own_lo.push_back(s.own_lo);
    h->own_rows.push_back(s.own_hi - s.own_lo + 1);
    h->view0.push_back(v0);
    h->timing = h->timing && p->timing;
    h->rows = P;
    h->ncp = x->g.ncp;
  }
  *out = h;
  return 0;
}

extern "C" void wdpm_group_ponds_destroy(wdpm_group_ponds *h) {
  if (!h) return;
  for (wdpm_ponds *p : h->r) destroy_handle(p);
  delete h;
}

extern "C" int wdpm_group_ponds_label(wdpm_group_ponds *h, double min_depth, int64_t *nponds) {
  if (!h) return wdpm_fail("wdpm_group_ponds_label: null handle");
  if (check_min_depth("wdpm_group_ponds_label", min_depth)) return 1;
  return group_label(h, min_depth, nponds, nullptr);
}

int wdpm_pond_detail::group_drain(wdpm_group_ponds *h) {
  std::string msg = wdpm_last_error();
  for (wdpm_ponds *p : h->r)
    if (hipSetDevice(p->x->p.device) == hipSuccess) (void)hipStreamSynchronize(p->x->stream);
  return wdpm_fail("%s", msg.c_str());
}

int wdpm_pond_detail::group_label(wdpm_group_ponds *h, double min_depth, int64_t *nponds, group_rims_queue rims,
                                  group_seams_queue seam_rows) {
  h->lab.valid = false;
  h->rim.valid = false;             /* a rim table belongs to the label call that made it */
  h->cat.valid = false;             /* and so does a catchment table */
  h->out.valid = false;             /* and an outlet table */
  h->cur.valid = false;             /* and a curve table */
  const int n = h->n;
  /* every rank up to its scan, on its own stream and device, before the first wait */
  for (int i = 0; i < n; i++)
    if (label_queue(h->r[i], min_depth) || (seam_rows && seam_rows(h, i))) return group_drain(h);
  std::vector<wdpm_stitch::RankSeams> seams((size_t)n);
  bool bad = false;
  std::string first_msg;
  for (int i = 0; i < n; i++) {
    long long ni = 0;
    if (label_status(h->r[i], &ni)) {           /* go on waiting for the others: nothing stays queued behind a failure */
      if (!bad) first_msg = wdpm_last_error();
      bad = true;
      continue;
    }
    seams[i].n = ni;
    seams[i].top = h->r[i]->lab.h_seam.p;
    seams[i].bottom = h->r[i]->lab.h_seam.p + h->ncp;
  }
  if (bad) return wdpm_fail("%s", first_msg.c_str());

  timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  wdpm_stitch::Result res;
  std::string err;
  if (wdpm_stitch::stitch(seams, h->ncp, res, err)) return wdpm_fail("wdpm_group_ponds_label: %s", err.c_str());
  clock_gettime(CLOCK_MONOTONIC, &t1);

  /* every rank's table kernel, its labels written once as whole-raster numbers, and its own table on the way to the host:
   * all of it queued (pinned staging on both ways) before the first wait */
  for (int i = 0; i < n; i++) {
    if (table_queue(h->r[i], true, res.map[i].data())) return group_drain(h);
    if (rims && rims(h, i, res.map, res.ponds)) return group_drain(h);
  }
  for (int i = 0; i < n; i++)
    if (table_wait(h->r[i])) {
      if (!bad) first_msg = wdpm_last_error();
      bad = true;
    }
  if (bad) return wdpm_fail("%s", first_msg.c_str());

  h->lab.rows.assign((size_t)res.ponds, wdpm_pond());
  for (int i = 0; i < n; i++)
    if (wdpm_stitch::fold_table(h->r[i]->lab.h_table.p, res.map[i], h->view0[i], h->lab.rows.data(), err))
      return wdpm_fail("wdpm_group_ponds_label: %s", err.c_str());

  h->lab.stats.ranks = n;
  h->lab.stats.ponds = res.ponds;
  h->lab.stats.local_ponds = res.local_ponds;
  h->lab.stats.stitch_unions = res.unions;
  h->lab.stats.merged = res.merged;
  h->lab.stats.stitch_ms = ms_between(t0, t1);
  h->lab.valid = true;
  if (nponds) *nponds = res.ponds;
  return 0;
}

extern "C" int wdpm_group_ponds_table(wdpm_group_ponds *h, wdpm_pond *out, int64_t capacity) {
  return table_out("wdpm_group_ponds_table", h, &wdpm_group_ponds::lab, kNoGroupTable, out, capacity);
}

extern "C" int wdpm_group_ponds_labels(wdpm_group_ponds *h, int32_t *padded) {
  if (!h || !padded) return wdpm_fail("wdpm_group_ponds_labels: null argument");
  if (!h->lab.valid) return wdpm_fail("wdpm_group_ponds_labels: %s", kNoGroupTable);
  /* Every rank's owned rows, to where they lie in the whole raster.  The caller's raster is pageable memory, to which a copy is
   * synchronous whatever it is called: the ranks' rows come down one after another, as wdpm_group_download_water's do. */
  for (int i = 0; i < h->n; i++) {
    wdpm_ponds *p = h->r[i];
    if (download(p, padded + (size_t)h->own_lo[i] * h->ncp, p->lab.labels.p + (size_t)(h->own_lo[i] - h->view0[i]) * h->ncp,
                 (size_t)h->own_rows[i] * h->ncp * sizeof(int32_t)))
      return 1;
  }
  return 0;
}

extern "C" int wdpm_group_ponds_guard_bad(wdpm_group_ponds *h, int64_t *bytes) {
  if (!h || !bytes) return wdpm_fail("wdpm_group_ponds_guard_bad: null argument");
  *bytes = 0;
  for (wdpm_ponds *p : h->r)
    if (count_guard_bad(p, bytes)) return 1;
  return 0;
}

extern "C" int wdpm_group_ponds_stats(wdpm_group_ponds *h, wdpm_group_pond_stats *out) {
  return stats_out("wdpm_group_ponds_stats", h, &wdpm_group_ponds::lab, kNoGroupTable, out, true);
}

extern "C" int wdpm_group_ponds_rank_stats(wdpm_group_ponds *h, int32_t rank, wdpm_pond_stats *out) {
  if (!h || !out) return wdpm_fail("wdpm_group_ponds_rank_stats: null argument");
  if (rank < 0 || rank >= h->n) return wdpm_fail("wdpm_group_ponds_rank_stats: rank %d of %d", rank, h->n);
  if (!h->lab.valid) return wdpm_fail("wdpm_group_ponds_rank_stats: %s", kNoGroupTable);
  *out = h->r[rank]->lab.stats;
  return 0;
}

extern "C" int wdpm_group_ponds_phase_ms(wdpm_group_ponds *h, int32_t rank, double *ms) {
  return group_phase_ms_out("wdpm_group_ponds_phase_ms", h, &wdpm_group_ponds::lab, &wdpm_ponds::lab, kNoGroupTable, rank, ms, true);
}
#endif  /* WDPM_PONDS_EMULATION */
