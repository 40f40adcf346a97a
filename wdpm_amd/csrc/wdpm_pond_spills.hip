/*
 * wdpm_pond_spills.hip — where every pond's overflow ends up (include/wdpm_pond_spills.h): the graph of the outlet table's to_basin
 * column followed downstream by pointer doubling over the tables a wdpm_curves_label leaves on the device.  gfx950.  A unit of its
 * own beside the six older ones: not in the launch ledger, not among the sources wdpm_build_info() hashes.
 *
 * One lane per pond, over flat arrays of N words each (SpillArrays); no raster is read.  Every pass runs R = spill_rounds(N) launches
 * whatever the graph, and a round reads one set of buffers and writes the other, so no lane reads what another lane of the same
 * launch writes.  work[pass][r] (SpillStatus) says whether round r has anything to do: the launch before it sets the word, a round
 * that finds 0 returns at once - every lane of it, the word is one for the whole grid - and so does every later one.  The host
 * waits for nothing between the launches, and no loop anywhere runs until a condition holds: a ring cannot keep one alive.
 *
 *   init     next = to_basin, the spilling flag, cells + catch_cells and fill_q, gathered from the four tables
 *   rings    per pond a pointer p (the pond 2^r steps on, 0: the chain ended before) and the smallest label m among the ponds 1..2^r
 *            steps on - the pond itself NOT among them.  A round: m = min(m, m[p]), p = p[p].  Only a pond on a ring meets itself
 *            again, and a ring is all a pond on it can reach, so after 2^R >= 2 N steps m == k exactly at the ring heads.  If a round
 *            changes no m, no later round would (m[p] >= m for every pond then holds along every path): the next ones are idle
 *   cut      next = -2 at the heads; the head's successor is marked: a pond lies on a ring exactly if that mark is in its subtree
 *   chains   over the forest, per pond a link (> 0: the pond exactly 2^r steps on; < 0: minus the last pond of a chain that ended
 *            before), the hops so far and the sum of fill_q over the ponds left behind.  A round: hops += hops[link], sum +=
 *            sum[link], link = link[link].  The same over the live forest, where only spilling ponds keep their edge: rest and
 *            rest_hops.  A round whose links are all ends leaves nothing to do
 *   sums     A_r(v), the sum over v's descendants within 2^r - 1 edges, becomes A_r+1(v) = A_r(v) + the A_r(u) of all u whose link
 *            of round r is v: every pond adds its A_r to its own word and to its link's word of the other buffer, with 64-bit
 *            integer atomics - any order gives the same bits - and clears the word it read, which is the target of the round after
 *            next.  Three sums over the forest's links, two over the live forest's; the links are doubled again beside them, in
 *            the buffers the ring pass no longer needs.  up_ponds < 2^31, so its word carries the ring mark's sum above bit 32
 *   finish   the rows; the counts of wdpm_spill_stats per wave before their atomics go out
 *
 * A hub - one pond fed by very many - would take one atomic per feeder and sum in the first round of `sums`, all on the same words
 * (measured: 90 778 direct feeders made that phase 2.5 ms of 3.0 for 128 919 ponds).  So the lanes of a wave that share a target are
 * summed by a butterfly first and send one atomic together (push_group).
 *
 * Everything that steers a loop or a return is wave-uniform.  tests/spills_emu_main.cpp compiles the kernels for the host under
 * sanitizers with WDPM_PONDS_EMULATION defined, as tests/curves_emu_main.cpp does with wdpm_pond_curves.hip, and leaves the host half
 * out.
 */
#include "wdpm_ponds_priv.h"

using namespace wdpm_pond_detail;

namespace {

constexpr int kRing = 0, kChain = 1, kSums = 2;   /* the rows of SpillStatus.work */
constexpr int kNoLabel = 0x7fffffff;              /* above every label */
constexpr int kAccs = 5;                          /* up_ponds (with the ring mark), up_cells, up_fill_q | live_ponds, live_cells */
constexpr int kForestAccs = 3;

/* N words each.  next: to_basin, -2 at a ring head once cut.  ptr / low: the ring pass's pointer and minimum; the sums pass's links
 * over the forest and over the live forest.  acc[b]: kAccs x N. */
struct SpillArrays {
  int *next, *flag, *mark;
  int *ptr[2], *low[2];
  int *link[2], *hops[2], *llink[2], *lhops[2];
  unsigned long long *cells, *fq, *path[2], *acc[2];
};
constexpr int kSpillWords = 15, kSpillSums = 4 + 2 * kAccs;   /* int and 64-bit arrays of N */

/* one lane of the wave stores the word when any lane asks for it; every lane takes part in the vote */
__device__ __forceinline__ void wave_flag(unsigned *w, bool any) {
  if (__ballot(any) != 0ull && (threadIdx.x & 63) == 0) __hip_atomic_store(w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool round_has_work(const SpillStatus *st, int pass, int r) {
  return __hip_atomic_load(&st->work[pass][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
}
/* the rounds of a pass that ran: its results lie in buffer (that number & 1) */
__device__ __forceinline__ int rounds_run(const SpillStatus *st, int pass, int rounds) {
  int r = 0;
  while (r < rounds && round_has_work(st, pass, r)) r++;
  return r;
}
__device__ __forceinline__ unsigned long long spill_wave_sum(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

/* ---- init ------------------------------------------------------------------------------------------------------------------ */
__global__ __launch_bounds__(kBlock) void spill_init_kernel(long long n, const wdpm_pond *__restrict__ ponds, const wdpm_pond_rim *__restrict__ rims,
                                                            const wdpm_pond_catchment *__restrict__ cat, const wdpm_pond_outlet *__restrict__ outlets,
                                                            double tol, SpillArrays a, SpillStatus *st) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < n;
  int to = -1;
  if (live) {
    to = outlets[i].to_basin;
    const double headroom = outlets[i].pour_level - rims[i].surface_max;      /* one fp64 subtraction; +inf without an outlet */
    a.next[i] = to;
    a.flag[i] = to >= 0 && headroom <= tol;
    a.mark[i] = 0;
    a.cells[i] = (unsigned long long)(ponds[i].cells + cat[i].catch_cells);
    a.fq[i] = outlets[i].fill_q;
    a.ptr[0][i] = to > 0 ? to : 0;
    a.low[0][i] = to > 0 ? to : kNoLabel;
  }
  wave_flag(&st->work[kRing][0], live && to > 0);
}

/* ---- rings ----------------------------------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(kBlock) void spill_ring_kernel(long long n, int r, SpillArrays a, SpillStatus *st) {
  if (!round_has_work(st, kRing, r)) return;
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < n;
  const int *__restrict__ pi = a.ptr[r & 1], *__restrict__ mi = a.low[r & 1];
  bool changed = false;
  if (live) {
    int p = pi[i], m = mi[i];
    if (p > 0) {
      const int m2 = mi[p - 1];
      p = pi[p - 1];
      changed = m2 < m;
      m = changed ? m2 : m;
    }
    a.ptr[(r + 1) & 1][i] = p;
    a.low[(r + 1) & 1][i] = m;
  }
  wave_flag(&st->work[kRing][r + 1], changed);
}

/* the heads leave their ring: only the head writes its own next, and the mark of its successor, which no other head shares */
__global__ __launch_bounds__(kBlock) void spill_cut_kernel(long long n, int rounds, SpillArrays a, const SpillStatus *st) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int *__restrict__ low = a.low[rounds_run(st, kRing, rounds) & 1];
  if (low[i] == (int)i + 1) {
    a.mark[a.next[i] - 1] = 1;
    a.next[i] = -2;
  }
}

/* ---- chains ---------------------------------------------------------------------------------------------------------------- */
/* the links of round 0 over the forest and over the live forest: the next pond, or minus the pond itself where its chain ends */
__device__ __forceinline__ void first_links(const SpillArrays &a, long long i, int &link, int &llink) {
  const int to = a.next[i];
  link = to > 0 ? to : -(int)(i + 1);
  llink = to > 0 && a.flag[i] ? to : -(int)(i + 1);
}

__global__ __launch_bounds__(kBlock) void spill_chain_init_kernel(long long n, SpillArrays a, SpillStatus *st) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < n;
  int link = 0, llink = 0;
  if (live) {
    first_links(a, i, link, llink);
    a.link[0][i] = link;
    a.hops[0][i] = link > 0;
    a.path[0][i] = link > 0 ? a.fq[i] : 0ull;
    a.llink[0][i] = llink;
    a.lhops[0][i] = llink > 0;
  }
  wave_flag(&st->work[kChain][0], live && link > 0);
}

__global__ __launch_bounds__(kBlock) void spill_chain_kernel(long long n, int r, SpillArrays a, SpillStatus *st) {
  if (!round_has_work(st, kChain, r)) return;
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < n;
  const int in = r & 1, out = in ^ 1;
  int link = 0;
  if (live) {
    link = a.link[in][i];
    int hops = a.hops[in][i];
    unsigned long long path = a.path[in][i];
    if (link > 0) {
      hops += a.hops[in][link - 1];
      path += a.path[in][link - 1];
      link = a.link[in][link - 1];
    }
    a.link[out][i] = link;
    a.hops[out][i] = hops;
    a.path[out][i] = path;
    int llink = a.llink[in][i], lhops = a.lhops[in][i];
    if (llink > 0) {
      lhops += a.lhops[in][llink - 1];
      llink = a.llink[in][llink - 1];
    }
    a.llink[out][i] = llink;
    a.lhops[out][i] = lhops;
  }
  wave_flag(&st->work[kChain][r + 1], live && link > 0);       /* a live link 2^r steps on has a forest link beside it */
}

/* ---- sums ------------------------------------------------------------------------------------------------------------------ */
__global__ __launch_bounds__(kBlock) void spill_sums_init_kernel(long long n, SpillArrays a, SpillStatus *st) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < n;
  int link = 0, llink = 0;
  if (live) {
    first_links(a, i, link, llink);
    a.ptr[0][i] = link;
    a.low[0][i] = llink;
    const unsigned long long cells = a.cells[i];
    a.acc[0][0 * n + i] = 1ull | ((unsigned long long)a.mark[i] << 32);
    a.acc[0][1 * n + i] = cells;
    a.acc[0][2 * n + i] = a.fq[i];
    a.acc[0][3 * n + i] = 1ull;
    a.acc[0][4 * n + i] = cells;
#pragma unroll
    for (int j = 0; j < kAccs; j++) a.acc[1][j * n + i] = 0ull;
  }
  wave_flag(&st->work[kSums][0], live && link > 0);
}

/* The pushes of one group of sums (those over the forest's links, or those over the live forest's): v[first..first + count) of every
 * lane with a target go to the target's words.  A hub - one pond fed by very many - would take all of these on the same words, so
 * the lanes of a wave that share a target go together first: up to kHubTries times the target of the first lane still waiting is
 * put to the vote, and where at least kHubLanes lanes hold it, one butterfly sum per word and ONE add stand for all of them (the
 * table kernel's by-label scheme, bounded).  Whoever is left adds for itself.  Integer sums: any grouping gives the same bits.
 * Every lane of the wave comes here; the votes and what follows from them are wave-uniform. */
constexpr int kHubTries = 3, kHubLanes = 8;

__device__ __forceinline__ void push_group(unsigned long long *to, long long n, int first, int count, int target,
                                           const unsigned long long (&v)[kAccs], int lane) {
  bool waiting = target > 0;
  int tried = 0;
  for (int t = 0; t < kHubTries; t++) {
    const unsigned long long pending = __ballot(waiting && target != tried);
    if (pending == 0ull) break;
    tried = __shfl(target, __builtin_ctzll(pending));
    const bool same = waiting && target == tried;
    if (__popcll(__ballot(same)) < kHubLanes) continue;
#pragma unroll
    for (int j = 0; j < kAccs; j++) {
      if (j < first || j >= first + count) continue;
      const unsigned long long sum = spill_wave_sum(same ? v[j] : 0ull);
      if (lane == 0 && sum != 0ull) atomicAdd(&to[j * n + (tried - 1)], sum);
    }
    waiting = waiting && !same;
  }
  if (waiting) {
#pragma unroll
    for (int j = 0; j < kAccs; j++)
      if (j >= first && j < first + count && v[j] != 0ull) atomicAdd(&to[j * n + (target - 1)], v[j]);
  }
}

__global__ __launch_bounds__(kBlock) void spill_sums_kernel(long long n, int r, SpillArrays a, SpillStatus *st) {
  if (!round_has_work(st, kSums, r)) return;
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < n;
  const int in = r & 1, out = in ^ 1;
  int link = 0, llink = 0;
  unsigned long long v[kAccs] = {0ull, 0ull, 0ull, 0ull, 0ull};
  unsigned long long *to = a.acc[out];
  if (live) {
    link = a.ptr[in][i];
    llink = a.low[in][i];
    unsigned long long *__restrict__ from = a.acc[in];
#pragma unroll
    for (int j = 0; j < kAccs; j++) {
      v[j] = from[j * n + i];
      from[j * n + i] = 0ull;                                  /* only this lane touches the word in this round */
      if (v[j] != 0ull) atomicAdd(&to[j * n + i], v[j]);       /* its own word of the other buffer, which its feeders add to as well */
    }
  }
  push_group(to, n, 0, kForestAccs, link, v, threadIdx.x & 63);
  push_group(to, n, kForestAccs, kAccs - kForestAccs, llink, v, threadIdx.x & 63);
  if (live) {
    a.low[out][i] = llink > 0 ? a.low[in][llink - 1] : llink;
    link = link > 0 ? a.ptr[in][link - 1] : link;
    a.ptr[out][i] = link;
  }
  wave_flag(&st->work[kSums][r + 1], live && link > 0);
}

/* ---- finish ---------------------------------------------------------------------------------------------------------------- */
/* every lane stays for the counts */
__global__ __launch_bounds__(kBlock) void spill_finish_kernel(long long n, int rounds, SpillArrays a, wdpm_pond_spill *__restrict__ table, SpillStatus *st) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < n;
  const int bc = rounds_run(st, kChain, rounds) & 1, bs = rounds_run(st, kSums, rounds) & 1;
  bool head = false, ring = false, spills = false, land = false, none = false;
  unsigned long long hops = 0ull;
  if (live) {
    const int self = (int)i + 1, next = a.next[i];
    const int link = a.link[bc][i], llink = a.llink[bc][i];
    const int sink = link < 0 ? -link : self, rest = llink < 0 ? -llink : self;     /* every link is an end by now */
    const unsigned long long *__restrict__ acc = a.acc[bs];
    const unsigned long long packed = acc[0 * n + i];
    wdpm_pond_spill row;
    row.next = next;
    row.sink = sink;
    row.end = a.next[sink - 1];
    row.hops = a.hops[bc][i];
    row.rest = rest;
    row.rest_hops = a.lhops[bc][i];
    row.spilling = a.flag[i];
    row.reserved = 0;
    row.path_fill_q = a.path[bc][i] + a.fq[sink - 1];
    row.up_ponds = (long long)(packed & 0xffffffffull);
    row.up_cells = (long long)acc[1 * n + i];
    row.up_fill_q = acc[2 * n + i];
    row.live_ponds = (long long)acc[3 * n + i];
    row.live_cells = (long long)acc[4 * n + i];
    table[i] = row;
    head = next == -2;
    ring = (packed >> 32) != 0ull;
    spills = row.spilling != 0;
    land = next == 0;
    none = next == -1;
    hops = (unsigned long long)row.hops;
  }
  const unsigned long long headm = __ballot(head), ringm = __ballot(ring), spillm = __ballot(spills), landm = __ballot(land), nonem = __ballot(none);
  hops = wave_max(hops);
  if ((threadIdx.x & 63) == 0) {
    if (headm) {
      atomicAdd(&st->rings, (unsigned long long)__popcll(headm));
      atomicAdd(&st->ends_ring, (unsigned long long)__popcll(headm));
    }
    if (ringm) atomicAdd(&st->ring_ponds, (unsigned long long)__popcll(ringm));
    if (spillm) atomicAdd(&st->spilling, (unsigned long long)__popcll(spillm));
    if (landm) atomicAdd(&st->ends_land, (unsigned long long)__popcll(landm));
    if (nonem) atomicAdd(&st->ends_none, (unsigned long long)__popcll(nonem));
    if (hops) atomic_max_if(&st->max_hops, hops);
  }
}

/* the arrays laid out in two buffers of kSpillWords x N ints and kSpillSums x N 64-bit words */
inline SpillArrays spill_arrays(int *words, unsigned long long *sums, long long n) {
  SpillArrays a;
  int **w[kSpillWords] = {&a.next, &a.flag, &a.mark, &a.ptr[0], &a.ptr[1], &a.low[0], &a.low[1], &a.link[0], &a.link[1], &a.hops[0], &a.hops[1],
                          &a.llink[0], &a.llink[1], &a.lhops[0], &a.lhops[1]};
  for (int j = 0; j < kSpillWords; j++) *w[j] = words + j * n;
  a.cells = sums;
  a.fq = sums + n;
  a.path[0] = sums + 2 * n;
  a.path[1] = sums + 3 * n;
  a.acc[0] = sums + 4 * n;
  a.acc[1] = sums + (4 + kAccs) * n;
  return a;
}

}  // namespace

#ifndef WDPM_PONDS_EMULATION
/* ---- host ------------------------------------------------------------------------------------------------------------------ */
namespace {
const char kNoTable[] = "no spill table: the last label call on this handle was not a wdpm_spill_label that succeeded";
}  // namespace

extern "C" int wdpm_spill_label(wdpm_ponds *h, double min_depth, double headroom_tol, int64_t *nponds) {
  if (!h) return wdpm_fail("wdpm_spill_label: null handle");
  if (check_min_depth("wdpm_spill_label", min_depth)) return 1;
  if (!(headroom_tol >= 0.0) || std::isinf(headroom_tol))
    return wdpm_fail("wdpm_spill_label: headroom_tol must be finite and >= 0 (got %g)", headroom_tol);
  if (h->seams) return wdpm_fail("wdpm_spill_label: the handle views a row block: spills are taken on whole rasters only");
  int64_t n = 0;
  if (wdpm_curves_label(h, min_depth, &n)) return 1;          /* leaves the four tables finished on the device and the stream as this pass wants it */
  h->lab.valid = false;                                       /* a wdpm_spill_label that fails leaves no table of any kind */
  wdpm_ctx *x = h->x;
  const hipStream_t sm = x->stream;
  HIP_TRY(hipSetDevice(x->p.device));
  const char *what;
  hipError_t e = ensure(h->spl.status, &what);
  if (e != hipSuccess) return wdpm_fail("wdpm_spill_label: no %s memory for the status words: %s", what, hipGetErrorString(e));
  e = grow(h, h->spl.table, n);                               /* sized from N, like the pond table */
  if (e == hipSuccess) e = grow(h, h->spl.words, (long long)kSpillWords * n);
  if (e == hipSuccess) e = grow(h, h->spl.sums, (long long)kSpillSums * n);
  if (e != hipSuccess) return wdpm_fail("wdpm_spill_label: no device memory for the spills of %lld ponds: %s", (long long)n, hipGetErrorString(e));
  h->spl.timer.clear();
  memset(h->spl.status.h, 0, sizeof(SpillStatus));
  const int rounds = n > 0 ? spill_rounds(n) : 0;
  if (n > 0) {                                                /* no pond, no spill: nothing to launch */
    const SpillArrays a = spill_arrays(h->spl.words.p, h->spl.sums.p, n);
    SpillStatus *st = h->spl.status.d;
    const dim3 grid(blocks_for(n, kBlock)), block(kBlock);
    HIP_TRY(hipMemsetAsync(st, 0, sizeof(SpillStatus), sm));
    HIP_TRY(h->spl.timer.mark(h->timing, 0, sm));
    hipLaunchKernelGGL(spill_init_kernel, grid, block, 0, sm, (long long)n, reinterpret_cast<const wdpm_pond *>(h->lab.table.p),
                       reinterpret_cast<const wdpm_pond_rim *>(h->rim.table.p), reinterpret_cast<const wdpm_pond_catchment *>(h->cat.table.p),
                       reinterpret_cast<const wdpm_pond_outlet *>(h->out.table.p), headroom_tol, a, st);
    for (int r = 0; r < rounds; r++) hipLaunchKernelGGL(spill_ring_kernel, grid, block, 0, sm, (long long)n, r, a, st);
    hipLaunchKernelGGL(spill_cut_kernel, grid, block, 0, sm, (long long)n, rounds, a, st);
    HIP_TRY(h->spl.timer.mark(h->timing, 1, sm));
    hipLaunchKernelGGL(spill_chain_init_kernel, grid, block, 0, sm, (long long)n, a, st);
    for (int r = 0; r < rounds; r++) hipLaunchKernelGGL(spill_chain_kernel, grid, block, 0, sm, (long long)n, r, a, st);
    HIP_TRY(h->spl.timer.mark(h->timing, 2, sm));
    hipLaunchKernelGGL(spill_sums_init_kernel, grid, block, 0, sm, (long long)n, a, st);
    for (int r = 0; r < rounds; r++) hipLaunchKernelGGL(spill_sums_kernel, grid, block, 0, sm, (long long)n, r, a, st);
    hipLaunchKernelGGL(spill_finish_kernel, grid, block, 0, sm, (long long)n, rounds, a, h->spl.table.p, st);
    HIP_TRY(h->spl.timer.mark(h->timing, 3, sm));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->spl.status.h, st, sizeof(SpillStatus), hipMemcpyDeviceToHost, sm));
    if (wdpm_stream_sync(x, sm)) return 1;
    if (h->timing) HIP_TRY(h->spl.timer.read_all());
  }
  const SpillStatus &s = *h->spl.status.h;
  h->spl.stats.ponds = n;
  h->spl.stats.rings = (int64_t)s.rings;
  h->spl.stats.ring_ponds = (int64_t)s.ring_ponds;
  h->spl.stats.spilling = (int64_t)s.spilling;
  h->spl.stats.ends_land = (int64_t)s.ends_land;
  h->spl.stats.ends_none = (int64_t)s.ends_none;
  h->spl.stats.ends_ring = (int64_t)s.ends_ring;
  h->spl.stats.max_hops = (int64_t)s.max_hops;
  h->spl.stats.rounds = (int64_t)kSpillPasses * rounds;
  h->spl.valid = true;
  h->lab.valid = true;
  if (nponds) *nponds = n;
  return 0;
}

extern "C" int wdpm_spill_table(wdpm_ponds *h, wdpm_pond_spill *out, int64_t capacity) {
  return table_out("wdpm_spill_table", h, &wdpm_ponds::spl, kNoTable, out, capacity);
}

extern "C" int wdpm_spill_stats(wdpm_ponds *h, wdpm_pond_spill_stats *out) {
  return stats_out("wdpm_spill_stats", h, &wdpm_ponds::spl, kNoTable, out);
}

extern "C" int wdpm_spill_phase_ms(wdpm_ponds *h, double *ms) {
  return phase_ms_out("wdpm_spill_phase_ms", h, &wdpm_ponds::spl, kNoTable, ms);
}
#endif  /* WDPM_PONDS_EMULATION */
