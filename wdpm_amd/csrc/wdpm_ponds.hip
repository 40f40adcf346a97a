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
 * address and undefined-behaviour sanitizers on) with WDPM_PONDS_EMULATION defined: it brings its own stand-ins for the HIP
 * device language and leaves the host half of this file out. */
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
#include "../../include/wdpm_ponds.h"

namespace {

constexpr int kSeg = 64;             /* columns per segment = lanes per wave */
constexpr int kBlock = 256;          /* threads per block: four waves, four segments */
constexpr int kWaves = kBlock / kSeg;
constexpr int kScanItems = 4;        /* segments per thread of the scan kernels */
constexpr int kScanTile = kBlock * kScanItems;
constexpr int kTableWaves = 32768;   /* the table kernel aims at this many waves: bounds the atomics on one table row */

/* Rows one wave of the table kernel owns: about kTableWaves waves whatever the raster's size, or what the caller forces
 * (WDPM_PONDS_ROWS_PER_WAVE when the handle is made: tests and tuning).  The host and the host emulation both ask here. */
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

/* first bit of the run of `m` that holds bit `pos` (which is set) */
__device__ __forceinline__ int run_start(unsigned long long m, int pos) {
  const unsigned long long z = ~m & ((1ull << pos) - 1ull);
  return z ? 64 - __clzll((long long)z) : 0;
}
__device__ __forceinline__ int bit(unsigned long long m, int pos) { return (int)((m >> pos) & 1ull); }

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

__device__ __forceinline__ void atomic_min_if(int *p, int v) {
  if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > v) atomicMin(p, v);
}
__device__ __forceinline__ void atomic_max_if(int *p, int v) {
  if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v) atomicMax(p, v);
}
/* one lane sends a carry.  The extrema only move one way, so a look first spares the atomic that would change nothing. */
__device__ __forceinline__ void send(PondRow *table, const Carry &c) {
  PondRow *t = table + (c.label - 1);
  atomicAdd(&t->cells, c.cells);
  atomicAdd(&t->volume_q, c.vol);
  if (__hip_atomic_load(&t->depth_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < c.key) atomicMax(&t->depth_key, c.key);
  atomic_min_if(&t->row_min, c.row_min);
  atomic_max_if(&t->row_max, c.row_max);
  atomic_min_if(&t->col_min, c.col_min);
  atomic_max_if(&t->col_max, c.col_max);
}

/* A wave owns segment column s of rows [r0, r0 + rpw).  Everything that steers the loops below is wave-uniform. */
__global__ __launch_bounds__(kBlock) void ponds_table_kernel(const double *__restrict__ w, const unsigned long long *__restrict__ masks,
                                                             const int *__restrict__ parent, const int *__restrict__ base,
                                                             const unsigned long long *__restrict__ rootmask, Geom g, int rpw,
                                                             int nwaves, int *__restrict__ labels, PondRow *table) {
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
    int label = 0;
    if (wet && st == lane) {               /* a run start: where is its root among the roots? */
      const int root = parent[idx];
      const int rr = root / g.ncp, rc = root - rr * g.ncp;
      const int rseg = rr * g.nsc + rc / kSeg, rbit = rc % kSeg;
      label = base[rseg] + __popcll(rootmask[rseg] & ((1ull << rbit) - 1ull)) + 1;
      if (root == idx) { table[label - 1].first_row = r; table[label - 1].first_col = c; }
    }
    label = __shfl(label, st);
    if (!wet) label = 0;
    if (inside) labels[idx] = label;

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

}  // namespace

#ifndef WDPM_PONDS_EMULATION
namespace {
/* ---- host ------------------------------------------------------------------------------------------------------------------ */
struct Guarded { char *base; size_t bytes; };

}  // namespace

struct wdpm_ponds {
  wdpm_ctx *x;
  Geom g;
  size_t guard;                     /* bytes of each guard band (WDPM_GUARD_KB when the handle was made) */
  std::vector<Guarded> guards;
  bool allocated;
  unsigned long long *d_masks, *d_rootmask, *d_busum;
  int *d_parent, *d_labels, *d_cnt, *d_bsum;
  unsigned *d_ucnt;
  Status *d_status, *h_status;      /* h_status pinned */
  PondRow *d_table;
  long long table_cap;
  int nb;                           /* blocks of the scan */
  int forced_rpw;                   /* WDPM_PONDS_ROWS_PER_WAVE when the handle was made, 0: the library chooses */
  bool valid;                       /* the last label call succeeded */
  bool timing;                      /* WDPM_PONDS_TIMING=1 when the handle was made: HIP events around every kernel */
  hipEvent_t ev[WDPM_PONDS_PHASES + 2];   /* the host reads the status between scan and table: two marks there */
  double phase_ms[WDPM_PONDS_PHASES];
  wdpm_pond_stats stats;
};

namespace {

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

/* frees every buffer and leaves the handle as it was made */
void release(wdpm_ponds *h) {
  guarded_free(h, h->d_masks); guarded_free(h, h->d_rootmask); guarded_free(h, h->d_parent); guarded_free(h, h->d_labels);
  guarded_free(h, h->d_cnt); guarded_free(h, h->d_ucnt); guarded_free(h, h->d_bsum); guarded_free(h, h->d_busum);
  guarded_free(h, h->d_table);
  (void)hipFree(h->d_status);
  if (h->h_status) (void)hipHostFree(h->h_status);
  h->d_masks = h->d_rootmask = h->d_busum = nullptr;
  h->d_parent = h->d_labels = h->d_cnt = h->d_bsum = nullptr;
  h->d_ucnt = nullptr;
  h->d_status = h->h_status = nullptr;
  h->d_table = nullptr;
  h->table_cap = 0;
  h->allocated = false;
}

int allocate(wdpm_ponds *h) {
  if (h->allocated) return 0;
  const size_t cells = (size_t)h->g.rows * h->g.ncp, nseg = (size_t)h->g.nseg;
  h->nb = (int)((nseg + kScanTile - 1) / kScanTile);
  hipError_t e = guarded_malloc(h, (void **)&h->d_masks, nseg * sizeof(unsigned long long));
  if (e == hipSuccess) e = guarded_malloc(h, (void **)&h->d_rootmask, nseg * sizeof(unsigned long long));
  if (e == hipSuccess) e = guarded_malloc(h, (void **)&h->d_parent, cells * sizeof(int));
  if (e == hipSuccess) e = guarded_malloc(h, (void **)&h->d_labels, cells * sizeof(int));
  if (e == hipSuccess) e = guarded_malloc(h, (void **)&h->d_cnt, nseg * sizeof(int));
  if (e == hipSuccess) e = guarded_malloc(h, (void **)&h->d_ucnt, nseg * sizeof(unsigned));
  if (e == hipSuccess) e = guarded_malloc(h, (void **)&h->d_bsum, (size_t)h->nb * sizeof(int));
  if (e == hipSuccess) e = guarded_malloc(h, (void **)&h->d_busum, (size_t)h->nb * 2 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMalloc(&h->d_status, sizeof(Status));
  if (e == hipSuccess) e = hipHostMalloc(&h->h_status, sizeof(Status));
  if (e != hipSuccess) {
    release(h);                     /* what was taken so far: the next call starts from nothing again */
    return wdpm_fail("wdpm_ponds_label: device allocation failed: %s", hipGetErrorString(e));
  }
  h->allocated = true;
  return 0;
}

inline unsigned blocks_for(long long items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

}  // namespace

extern "C" int wdpm_ponds_create(wdpm_ponds **out, wdpm_ctx *ctx) {
  if (!out || !ctx) return wdpm_fail("wdpm_ponds_create: null argument");
  const SlabGeom &sg = ctx->g;
  if (sg.row0 != 0 || sg.rows != sg.R + 2)
    return wdpm_fail("wdpm_ponds_create: a slab context (rows %d..%d of %d) cannot take an inventory: ponds cross row blocks; "
                     "use a context that holds the whole raster", sg.row0, sg.row0 + sg.rows, sg.R + 2);
  if (wdpm_synchronize(ctx)) return 1;          /* binds the device */
  wdpm_ponds *h = new wdpm_ponds();
  h->x = ctx;
  h->g.rows = sg.rows;
  h->g.ncp = sg.ncp;
  h->g.nsc = (sg.ncp + kSeg - 1) / kSeg;
  h->g.nseg = h->g.rows * h->g.nsc;             /* <= cells / 64 + rows: an int with 2e9 cells */
  const char *e = getenv("WDPM_GUARD_KB");
  const long kb = e ? atol(e) : 0;
  h->guard = kb > 0 ? (size_t)kb * 1024 : 0;
  h->allocated = false;
  h->d_masks = h->d_rootmask = h->d_busum = nullptr;
  h->d_parent = h->d_labels = h->d_cnt = h->d_bsum = nullptr;
  h->d_ucnt = nullptr;
  h->d_status = h->h_status = nullptr;
  h->d_table = nullptr;
  h->table_cap = 0;
  h->nb = 0;
  { const char *re = getenv("WDPM_PONDS_ROWS_PER_WAVE"); h->forced_rpw = re ? atoi(re) : 0; }
  h->valid = false;
  memset(&h->stats, 0, sizeof h->stats);
  const char *te = getenv("WDPM_PONDS_TIMING");
  h->timing = te && atoi(te) != 0;
  for (int i = 0; i < WDPM_PONDS_PHASES + 2; i++) h->ev[i] = nullptr;
  for (int i = 0; i < WDPM_PONDS_PHASES; i++) h->phase_ms[i] = 0.0;
  if (h->timing)
    for (int i = 0; i < WDPM_PONDS_PHASES + 2; i++)
      if (hipEventCreate(&h->ev[i]) != hipSuccess) { h->timing = false; break; }
  *out = h;
  return 0;
}

extern "C" void wdpm_ponds_destroy(wdpm_ponds *h) {
  if (!h) return;
  (void)wdpm_synchronize(h->x);
  release(h);
  for (int i = 0; i < WDPM_PONDS_PHASES + 2; i++)
    if (h->ev[i]) (void)hipEventDestroy(h->ev[i]);
  delete h;
}

extern "C" int wdpm_ponds_label(wdpm_ponds *h, double min_depth, int64_t *nponds) {
  if (!h) return wdpm_fail("wdpm_ponds_label: null handle");
  if (!(min_depth >= 0.0) || std::isinf(min_depth)) return wdpm_fail("wdpm_ponds_label: min_depth must be finite and >= 0 (got %g)", min_depth);
  wdpm_ctx *x = h->x;
  h->valid = false;
  /* the raster as a reader sees it: side stream joined, owed drain() and threshold flush applied (what wdpm_count_stats asks for) */
  if (wdpm_synchronize(x)) return 1;
  if (wdpm_apply_owed_flush(x)) return 1;
  if (allocate(h)) return 1;
  const Geom g = h->g;
  const hipStream_t sm = x->stream;
  const double *w = x->d_w[x->cur];
  const unsigned seg_blocks = blocks_for(g.nseg, kWaves);

  HIP_TRY(hipMemsetAsync(h->d_status, 0, sizeof(Status), sm));
#define PONDS_MARK(i) do { if (h->timing) HIP_TRY(hipEventRecord(h->ev[i], sm)); } while (0)
  PONDS_MARK(0);
  hipLaunchKernelGGL(ponds_mask_kernel, dim3(seg_blocks), dim3(kBlock), 0, sm, w, x->d_dem, g, min_depth, h->d_masks, h->d_parent, h->d_status);
  PONDS_MARK(1);
  hipLaunchKernelGGL(ponds_merge_kernel, dim3(seg_blocks), dim3(kBlock), 0, sm, h->d_masks, h->d_parent, g, h->d_ucnt);
  PONDS_MARK(2);
  hipLaunchKernelGGL(ponds_flatten_kernel, dim3(seg_blocks), dim3(kBlock), 0, sm, h->d_masks, h->d_parent, g, h->d_cnt, h->d_rootmask);
  PONDS_MARK(3);
  hipLaunchKernelGGL(ponds_scan_reduce_kernel, dim3(h->nb), dim3(kBlock), 0, sm, h->d_cnt, h->d_ucnt, g.nseg, h->d_bsum, h->d_busum);
  hipLaunchKernelGGL(ponds_scan_sums_kernel, dim3(1), dim3(kBlock), 0, sm, h->d_bsum, h->d_busum, h->nb, h->d_status);
  hipLaunchKernelGGL(ponds_scan_down_kernel, dim3(h->nb), dim3(kBlock), 0, sm, h->d_cnt, g.nseg, h->d_bsum);
  PONDS_MARK(4);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h->h_status, h->d_status, sizeof(Status), hipMemcpyDeviceToHost, sm));
  if (wdpm_stream_sync(x, sm)) return 1;
  const Status st = *h->h_status;
  if (st.deep)
    return wdpm_fail("wdpm_ponds_label: a pond cell holds 512 m of water or more: volume_q (a 64-bit sum of depths in units of "
                     "2^-24 m) is only safe below that depth");
  const long long n = st.ponds;

  if (n > h->table_cap) {                       /* sized from N, now that N is known */
    guarded_free(h, h->d_table);
    h->d_table = nullptr;
    h->table_cap = 0;
    const hipError_t e = guarded_malloc(h, (void **)&h->d_table, (size_t)n * sizeof(PondRow));
    if (e != hipSuccess) return wdpm_fail("wdpm_ponds_label: no device memory for a table of %lld ponds: %s", n, hipGetErrorString(e));
    h->table_cap = n;
  }
  const int rpw = ponds_rows_per_wave(g.nseg, g.rows, h->forced_rpw);
  const int nwaves = ((g.rows + rpw - 1) / rpw) * g.nsc;
  PONDS_MARK(5);
  if (n > 0) hipLaunchKernelGGL(ponds_table_init_kernel, dim3(blocks_for(n, kBlock)), dim3(kBlock), 0, sm, h->d_table, n);
  hipLaunchKernelGGL(ponds_table_kernel, dim3(blocks_for(nwaves, kWaves)), dim3(kBlock), 0, sm, w, h->d_masks, h->d_parent, h->d_cnt,
                     h->d_rootmask, g, rpw, nwaves, h->d_labels, h->d_table);
  PONDS_MARK(6);
  if (n > 0) hipLaunchKernelGGL(ponds_table_finish_kernel, dim3(blocks_for(n, kBlock)), dim3(kBlock), 0, sm, h->d_table, n);
  PONDS_MARK(7);
#undef PONDS_MARK
  HIP_TRY(hipGetLastError());
  if (wdpm_stream_sync(x, sm)) return 1;
  if (h->timing) {
    /* mask, merge, flatten, scan, (host: status, table allocation), table init + table, finish */
    static const int from[WDPM_PONDS_PHASES] = {0, 1, 2, 3, 5, 6}, to[WDPM_PONDS_PHASES] = {1, 2, 3, 4, 6, 7};
    for (int i = 0; i < WDPM_PONDS_PHASES; i++) {
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, h->ev[from[i]], h->ev[to[i]]));
      h->phase_ms[i] = ms;
    }
  }

  h->stats.segments = g.nseg;
  h->stats.unions = (int64_t)st.unions;
  h->stats.seam_unions = (int64_t)st.seam_unions;
  h->stats.passes = 0;
  h->stats.rows_per_wave = rpw;
  h->stats.ponds = n;
  h->valid = true;
  if (nponds) *nponds = n;
  return 0;
}

extern "C" int wdpm_ponds_table(wdpm_ponds *h, wdpm_pond *out, int64_t capacity) {
  if (!h) return wdpm_fail("wdpm_ponds_table: null handle");
  if (!h->valid) return wdpm_fail("wdpm_ponds_table: no inventory: wdpm_ponds_label has not succeeded on this handle");
  const long long n = h->stats.ponds;
  if (capacity < n) return wdpm_fail("wdpm_ponds_table: capacity %lld is too small for %lld ponds", (long long)capacity, n);
  if (n == 0) return 0;
  if (!out) return wdpm_fail("wdpm_ponds_table: null output");
  if (wdpm_synchronize(h->x)) return 1;
  HIP_TRY(hipMemcpyAsync(out, h->d_table, (size_t)n * sizeof(wdpm_pond), hipMemcpyDeviceToHost, h->x->stream));
  return wdpm_stream_sync(h->x, h->x->stream);
}

extern "C" int wdpm_ponds_labels(wdpm_ponds *h, int32_t *padded) {
  if (!h || !padded) return wdpm_fail("wdpm_ponds_labels: null argument");
  if (!h->valid) return wdpm_fail("wdpm_ponds_labels: no inventory: wdpm_ponds_label has not succeeded on this handle");
  if (wdpm_synchronize(h->x)) return 1;
  HIP_TRY(hipMemcpyAsync(padded, h->d_labels, (size_t)h->g.rows * h->g.ncp * sizeof(int32_t), hipMemcpyDeviceToHost, h->x->stream));
  return wdpm_stream_sync(h->x, h->x->stream);
}

extern "C" int wdpm_ponds_guard_bad(wdpm_ponds *h, int64_t *bytes) {
  if (!h || !bytes) return wdpm_fail("wdpm_ponds_guard_bad: null argument");
  *bytes = 0;
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

extern "C" int wdpm_ponds_stats(wdpm_ponds *h, wdpm_pond_stats *out) {
  if (!h || !out) return wdpm_fail("wdpm_ponds_stats: null argument");
  if (!h->valid) return wdpm_fail("wdpm_ponds_stats: no inventory: wdpm_ponds_label has not succeeded on this handle");
  *out = h->stats;
  return 0;
}

extern "C" int wdpm_ponds_phase_ms(wdpm_ponds *h, double *ms) {
  if (!h || !ms) return wdpm_fail("wdpm_ponds_phase_ms: null argument");
  if (!h->timing) return wdpm_fail("wdpm_ponds_phase_ms: the handle records no events (set WDPM_PONDS_TIMING=1 before it is made)");
  if (!h->valid) return wdpm_fail("wdpm_ponds_phase_ms: no inventory: wdpm_ponds_label has not succeeded on this handle");
  for (int i = 0; i < WDPM_PONDS_PHASES; i++) ms[i] = h->phase_ms[i];
  return 0;
}
#endif  /* WDPM_PONDS_EMULATION */
