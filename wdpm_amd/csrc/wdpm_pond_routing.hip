/*
 * wdpm_pond_routing.hip — a runoff depth sent down the spill graph (include/wdpm_pond_routing.h): every pond takes runoff_q times its
 * basin's area and what the ponds above it pass on, keeps what its storage holds and passes on the rest.  gfx950.  A unit of its own
 * beside the seven older ones: not in the launch ledger, not among the sources wdpm_build_info() hashes.
 *
 * Overflow is max(0, ...), so the ponds are taken upstream first: level l = hops holds ponds that are independent of each other and
 * spill into level l - 1.  One lane per pond, over flat arrays of N words (RouteArrays); no raster is read.
 *
 *   order    once per label call.  init gathers next and hops from the spill table, cells + catch_cells and fill_q from the older
 *            tables, and counts the ponds of every level; scan turns the counts into offsets (one workgroup, a running carry);
 *            scatter writes the pond numbers into order[] level by level.  The lanes of a wave that share a level go to its counter
 *            together (level_slot).  Inside a level the order is whatever the atomics make it: every result is a sum of integers.
 *            The host fetches the levels + 1 offsets and plans the sweep (wdpm_route_plan.h)
 *   sweep    from the deepest level to level 0.  A level of more ponds than one workgroup is one grid launch; a run of consecutive
 *            smaller levels is one launch of ONE workgroup that walks them with a block barrier in between (none between two levels
 *            of at most 64 ponds, which are the first wave's alone) - its trip count is the host's, it waits for no condition and
 *            for no other workgroup.  A pond that overflows into another pond adds three
 *            words to it: out_q to in_q, and its reach_ponds and reach_cells.  The lanes of a wave that share a target are summed
 *            first (route_push, as push_group of wdpm_pond_spills.hip): one hub of 90 778 feeders lies on one level.  Overflow that
 *            leaves the graph - onto land, or at a ring head - goes to the status words, one add per wave
 *   finish   the rows, from the words the sweep left; the counts and totals of wdpm_pond_route_stats per wave before their atomics
 *
 * Inside a run a pond reads words that other waves of the same launch have added to one level earlier.  Those adds are agent-scope
 * atomics, performed in L2; every wave waits for its own (route_drain) before the block barrier; and the reads are relaxed
 * agent-scope atomic loads (fresh), which pass the CU's vector L1 - a plain load could be served from a line that L1 took before
 * the add (as in wdpm_ponds.hip and wdpm_pond_catchments.hip).  Between two levels that are one wave's alone there is no barrier:
 * the wave's wait for its own atomics stands between its adds and its next loads, which pass L1 all the same.  A rerun clears the three words and the status words on the stream
 * and runs sweep and finish again.
 *
 * Everything that steers a loop or a return is wave-uniform.  tests/routing_emu_main.cpp compiles the kernels for the host under
 * sanitizers with WDPM_PONDS_EMULATION defined and leaves the host half out.
 */
#include "wdpm_ponds_priv.h"

using namespace wdpm_pond_detail;

namespace {

constexpr int kRouteAccs = 3;                     /* in_q, reach_ponds, reach_cells: what the feeders add */
constexpr int kRouteWords = 3, kRouteSums = 2 + kRouteAccs;   /* int and 64-bit arrays of N */

/* N words each, but offsets (levels + 1) and cursor (levels).  order: the pond numbers 1..N by level, level 0 first. */
struct RouteArrays {
  int *next, *level, *order, *offsets, *cursor;
  unsigned long long *area, *fq, *acc;            /* acc: kRouteAccs x N */
};

__device__ __forceinline__ unsigned long long route_wave_sum(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}
/* a word that atomics of this launch may have added to */
__device__ __forceinline__ unsigned long long fresh(const unsigned long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
/* every atomic this wave has sent has been performed: before a barrier behind which another wave reads the word */
__device__ __forceinline__ void route_drain() {
#ifndef WDPM_PONDS_EMULATION
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#else
  wave_sync();                                    /* the lanes of a wave are host threads: here they are in step, as a wave always is */
#endif
}

/* ---- order ----------------------------------------------------------------------------------------------------------------- */
/* One add to counter[level] for every lane that is `live`, and - kWant - the lane's slot: what the counter held before, plus the
 * lane's rank among the lanes that went with it.  Up to kLevelTries times the level of the first lane still waiting is put to the
 * vote and ONE add stands for all the lanes that hold it; whoever is left adds for itself.  Every lane of the wave comes here. */
constexpr int kLevelTries = 4;

template <bool kWant>
__device__ __forceinline__ int level_slot(int *counter, int level, bool live, int lane) {
  bool waiting = live;
  int slot = 0;
  for (int t = 0; t < kLevelTries; t++) {
    const unsigned long long pending = __ballot(waiting);
    if (pending == 0ull) break;
    const int leader = __builtin_ctzll(pending);
    const int tried = __shfl(level, leader);
    const bool same = waiting && level == tried;
    const unsigned long long group = __ballot(same);
    int base = 0;
    if (lane == leader) base = atomicAdd(&counter[tried], __popcll(group));
    if (kWant) {
      base = __shfl(base, leader);
      if (same) slot = base + __popcll(group & ((1ull << lane) - 1ull));
    }
    waiting = waiting && !same;
  }
  if (waiting) slot = atomicAdd(&counter[level], 1);
  return slot;
}

/* a.offsets[0 .. levels] is zero on entry; on exit offsets[l] is the number of ponds of level l */
__global__ __launch_bounds__(kBlock) void route_init_kernel(long long n, const wdpm_pond *__restrict__ ponds, const wdpm_pond_catchment *__restrict__ cat,
                                                            const wdpm_pond_outlet *__restrict__ outlets, const wdpm_pond_spill *__restrict__ spills,
                                                            RouteArrays a) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < n;
  int level = 0;
  if (live) {
    level = spills[i].hops;
    a.next[i] = spills[i].next;
    a.level[i] = level;
    a.area[i] = (unsigned long long)(ponds[i].cells + cat[i].catch_cells);
    a.fq[i] = outlets[i].fill_q;
  }
  (void)level_slot<false>(a.offsets, level, live, threadIdx.x & 63);
}

/* One workgroup: the counts of levels 0 .. levels - 1 become their exclusive sums, offsets[levels] the total; cursor[l] starts at
 * offsets[l].  kBlock entries to a trip, the carry goes from trip to trip; the trip count is the host's. */
__global__ __launch_bounds__(kBlock) void route_scan_kernel(int levels, RouteArrays a) {
  __shared__ int wave_total[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;
  for (int base = 0; base <= levels; base += kBlock) {
    const int i = base + (int)threadIdx.x;
    const int v = i < levels ? a.offsets[i] : 0;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(incl, d);
      if (lane >= d) incl += t;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) {
      before += w < wave ? wave_total[w] : 0;
      total += wave_total[w];
    }
    const int excl = carry + before + incl - v;
    if (i <= levels) a.offsets[i] = excl;
    if (i < levels) a.cursor[i] = excl;
    carry += total;
    __syncthreads();                 /* wave_total is written again in the next trip */
  }
}

__global__ __launch_bounds__(kBlock) void route_scatter_kernel(long long n, RouteArrays a) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < n;
  const int level = live ? a.level[i] : 0;
  const int slot = level_slot<true>(a.cursor, level, live, threadIdx.x & 63);
  if (live) a.order[slot] = (int)i + 1;
}

/* ---- sweep ----------------------------------------------------------------------------------------------------------------- */
/* v[0 .. kRouteAccs) of every lane with a target go to the target's words.  Where fewer than kRouteHubLanes lanes push at all, each
 * adds for itself; otherwise up to kRouteHubTries times the target of the first lane still waiting is put to the vote, and where at
 * least kRouteHubLanes lanes hold it, one butterfly sum per word and ONE add stand for all of them.  Whoever is left adds for itself.
 * Integer sums: any grouping gives the same bits.  Every lane of the wave comes here; the votes are wave-uniform.  `votes`: the
 * level holds enough ponds for a vote to succeed at all - a run's level of fewer sends its adds without a look at the other lanes. */
constexpr int kRouteHubTries = 3, kRouteHubLanes = 8;

__device__ __forceinline__ void route_push(unsigned long long *to, long long n, int target, bool votes, const unsigned long long (&v)[kRouteAccs], int lane) {
  bool waiting = target > 0;
  if (votes && __popcll(__ballot(waiting)) >= kRouteHubLanes) {
    int tried = 0;
    for (int t = 0; t < kRouteHubTries; t++) {
      const unsigned long long pending = __ballot(waiting && target != tried);
      if (pending == 0ull) break;
      tried = __shfl(target, __builtin_ctzll(pending));
      const bool same = waiting && target == tried;
      if (__popcll(__ballot(same)) < kRouteHubLanes) continue;
#pragma unroll
      for (int j = 0; j < kRouteAccs; j++) {
        const unsigned long long sum = route_wave_sum(same ? v[j] : 0ull);
        if (lane == 0) atomicAdd(&to[j * n + (tried - 1)], sum);
      }
      waiting = waiting && !same;
    }
  }
  if (waiting) {
#pragma unroll
    for (int j = 0; j < kRouteAccs; j++) atomicAdd(&to[j * n + (target - 1)], v[j]);
  }
}

/* One pond (0: this lane has none) of the level under way: everything above it has been added to its words.  Every lane of a wave
 * that holds a pond of the level comes here; a wave that holds none stays away, which the caller knows from the level's size alone.
 * `sinks`: the level is level 0, whose ponds have next <= 0 - their overflow leaves the graph, and nothing is pushed; the ponds of
 * every other level have next > 0 (hops == 0 exactly where next <= 0: include/wdpm_pond_spills.h). */
__device__ __forceinline__ void route_step(int pond, bool sinks, bool votes, long long n, unsigned long long runoff_q, const RouteArrays &a, RouteStatus *st, int lane) {
  unsigned long long v[kRouteAccs] = {0ull, 0ull, 0ull};
  unsigned long long out = 0ull;
  int next = -1;
  if (pond > 0) {
    const long long k = pond - 1;
    next = a.next[k];
    const unsigned long long area = a.area[k], fill = a.fq[k];
    const unsigned long long all = runoff_q * area + fresh(&a.acc[k]);
    out = next != -1 && all > fill ? all - fill : 0ull;
    if (!sinks) {
      v[0] = out;
      v[1] = 1ull + fresh(&a.acc[n + k]);
      v[2] = area + fresh(&a.acc[2 * n + k]);
    }
  }
  if (!sinks) {
    route_push(a.acc, n, out != 0ull && next > 0 ? next : 0, votes, v, lane);
  } else if (__ballot(out != 0ull) != 0ull) {
    const unsigned long long land = route_wave_sum(next == 0 ? out : 0ull), ring = route_wave_sum(next == -2 ? out : 0ull);
    if (lane == 0) {
      if (land) atomicAdd(&st->out_land_q, land);
      if (ring) atomicAdd(&st->out_ring_q, ring);
    }
  }
}

/* a wide level: order[first .. first + count); the last block's waves past the level's end have nothing to do */
__global__ __launch_bounds__(kBlock) void route_level_kernel(int first, int count, bool sinks, long long n, unsigned long long runoff_q, RouteArrays a,
                                                             RouteStatus *st) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i - (threadIdx.x & 63) >= count) return;
  route_step(i < count ? a.order[first + i] : 0, sinks, true, n, runoff_q, a, st, threadIdx.x & 63);
}

/* A run: levels top, top - 1, ..., top - levels + 1, each of at most kBlock ponds, in ONE workgroup.  A level of at most 64 ponds is
 * the first wave's alone.  Between two levels the workgroup meets at a block barrier wherever more than one wave takes part in
 * either; between two levels of one wave that wave's own wait for its atomics orders them, and the other waves walk on to the next
 * barrier.  The sizes are the same for every wave, so all of them meet at the same barriers. */
__global__ __launch_bounds__(kBlock) void route_run_kernel(int top, int levels, long long n, unsigned long long runoff_q, RouteArrays a, RouteStatus *st) {
  const int wave_first = (int)threadIdx.x & ~63;
  int first = a.offsets[top], count = a.offsets[top + 1] - first;
  for (int j = 0; j < levels; j++) {
    const int level = top - j;
    if (wave_first < count) {
      route_step((int)threadIdx.x < count ? a.order[first + (int)threadIdx.x] : 0, level == 0, count >= kRouteHubLanes, n, runoff_q, a, st,
                 threadIdx.x & 63);
      route_drain();
    }
    if (j + 1 == levels) break;
    const int below = a.offsets[level - 1], below_count = first - below;
    if (count > kSeg || below_count > kSeg) __syncthreads();
    first = below;
    count = below_count;
  }
}

/* ---- finish ---------------------------------------------------------------------------------------------------------------- */
/* every lane stays for the counts */
__global__ __launch_bounds__(kBlock) void route_finish_kernel(long long n, unsigned long long runoff_q, RouteArrays a, wdpm_pond_route *__restrict__ table,
                                                              RouteStatus *st) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < n;
  unsigned long long own = 0ull, kept = 0ull;
  bool over = false, full = false;
  if (live) {
    const int next = a.next[i];
    const unsigned long long area = a.area[i], fill = a.fq[i], in = a.acc[i];
    own = runoff_q * area;
    const unsigned long long all = own + in;
    const unsigned long long out = next != -1 && all > fill ? all - fill : 0ull;
    kept = all - out;
    over = out != 0ull;
    full = next != -1 && all >= fill;
    wdpm_pond_route row;
    row.own_q = own;
    row.in_q = in;
    row.kept_q = kept;
    row.out_q = out;
    row.reach_ponds = (long long)(1ull + a.acc[n + i]);
    row.reach_cells = (long long)(area + a.acc[2 * n + i]);
    row.overflows = over;
    row.full = full;
    row.level = a.level[i];
    row.reserved = 0;
    table[i] = row;
  }
  const unsigned long long overm = __ballot(over), fullm = __ballot(full);
  own = route_wave_sum(own);
  kept = route_wave_sum(kept);
  if ((threadIdx.x & 63) == 0) {
    if (overm) atomicAdd(&st->overflowing, (unsigned long long)__popcll(overm));
    if (fullm) atomicAdd(&st->full, (unsigned long long)__popcll(fullm));
    if (own) atomicAdd(&st->own_q, own);
    if (kept) atomicAdd(&st->kept_q, kept);
  }
}

/* the arrays laid out in two buffers of kRouteWords x N + 2 (levels + 1) ints and kRouteSums x N 64-bit words */
inline RouteArrays route_arrays(int *words, unsigned long long *sums, long long n, int levels) {
  RouteArrays a;
  a.next = words;
  a.level = words + n;
  a.order = words + 2 * n;
  a.offsets = words + kRouteWords * n;
  a.cursor = a.offsets + levels + 1;
  a.area = sums;
  a.fq = sums + n;
  a.acc = sums + 2 * n;
  return a;
}

}  // namespace

#ifndef WDPM_PONDS_EMULATION
/* ---- host ------------------------------------------------------------------------------------------------------------------ */
namespace {
const char kNoTable[] = "no routing table: the last label call on this handle was not a wdpm_route_label that succeeded";

int check_runoff(const char *caller, double runoff_m, int64_t *q) {
  *q = wdpm_route_runoff_q(runoff_m);
  return *q < 0 ? wdpm_fail("%s: runoff_m must be finite, >= 0 and below 256 m (got %g)", caller, runoff_m) : 0;
}

/* sweep and finish for runoff_q on the order, the plan and the gathered arrays of the last label call: queued on the context's
 * stream behind a clearing of the words the sweep adds to, then the one wait */
int route_sweep(wdpm_ponds *h, long long n, int64_t runoff_q) {
  RouteUnit &u = h->rte;
  wdpm_ctx *x = h->x;
  const hipStream_t sm = x->stream;
  memset(u.status.h, 0, sizeof(RouteStatus));
  if (n > 0) {
    const RouteArrays a = route_arrays(u.words.p, u.sums.p, n, u.levels);
    RouteStatus *st = u.status.d;
    const dim3 block(kBlock);
    HIP_TRY(hipMemsetAsync(a.acc, 0, (size_t)kRouteAccs * n * sizeof(unsigned long long), sm));
    HIP_TRY(hipMemsetAsync(st, 0, sizeof(RouteStatus), sm));
    HIP_TRY(u.timer.mark(h->timing, 2, sm));
    for (const RouteLaunch &l : u.plan.launches) {
      if (l.wide)
        hipLaunchKernelGGL(route_level_kernel, dim3(blocks_for(l.count, kBlock)), block, 0, sm, l.first, l.count, l.top == 0, (long long)n,
                           (unsigned long long)runoff_q, a, st);
      else
        hipLaunchKernelGGL(route_run_kernel, dim3(1), block, 0, sm, l.top, l.levels, (long long)n, (unsigned long long)runoff_q, a, st);
    }
    HIP_TRY(u.timer.mark(h->timing, 3, sm));
    hipLaunchKernelGGL(route_finish_kernel, dim3(blocks_for(n, kBlock)), block, 0, sm, (long long)n, (unsigned long long)runoff_q, a, u.table.p, st);
    HIP_TRY(u.timer.mark(h->timing, 4, sm));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(u.status.h, st, sizeof(RouteStatus), hipMemcpyDeviceToHost, sm));
    if (wdpm_stream_sync(x, sm)) return 1;
    if (h->timing) {
      HIP_TRY(u.timer.read(2, 3, &u.timer.ms[1]));
      HIP_TRY(u.timer.read(3, 4, &u.timer.ms[2]));
    }
  }
  const RouteStatus &s = *u.status.h;
  u.stats.ponds = n;
  u.stats.runoff_q = runoff_q;
  u.stats.levels = u.levels;
  u.stats.wide_levels = u.plan.wide_levels;
  u.stats.launches = (int64_t)u.plan.launches.size();
  u.stats.overflowing = (int64_t)s.overflowing;
  u.stats.full = (int64_t)s.full;
  u.stats.own_q = s.own_q;
  u.stats.kept_q = s.kept_q;
  u.stats.out_land_q = s.out_land_q;
  u.stats.out_ring_q = s.out_ring_q;
  return 0;
}
}  // namespace

extern "C" int64_t wdpm_route_runoff_q(double runoff_m) {
  if (!(runoff_m >= 0.0) || std::isinf(runoff_m)) return -1;
  const double q = rint(ldexp(runoff_m, 24));
  return q < 4294967296.0 ? (int64_t)q : -1;
}

extern "C" int wdpm_route_label(wdpm_ponds *h, double min_depth, double headroom_tol, double runoff_m, int64_t *nponds) {
  if (!h) return wdpm_fail("wdpm_route_label: null handle");
  if (check_min_depth("wdpm_route_label", min_depth)) return 1;
  if (!(headroom_tol >= 0.0) || std::isinf(headroom_tol))
    return wdpm_fail("wdpm_route_label: headroom_tol must be finite and >= 0 (got %g)", headroom_tol);
  int64_t runoff_q = 0;
  if (check_runoff("wdpm_route_label", runoff_m, &runoff_q)) return 1;
  if (h->seams) return wdpm_fail("wdpm_route_label: the handle views a row block: routing is taken on whole rasters only");
  int64_t n = 0;
  if (wdpm_spill_label(h, min_depth, headroom_tol, &n)) return 1;   /* leaves the tables finished on the device, and max_hops on the host */
  h->lab.valid = false;                                       /* a wdpm_route_label that fails leaves no table of any kind */
  RouteUnit &u = h->rte;
  wdpm_ctx *x = h->x;
  const hipStream_t sm = x->stream;
  HIP_TRY(hipSetDevice(x->p.device));
  const int levels = n > 0 ? (int)h->spl.stats.max_hops + 1 : 0;
  const char *what;
  hipError_t e = ensure(u.status, &what);
  if (e != hipSuccess) return wdpm_fail("wdpm_route_label: no %s memory for the status words: %s", what, hipGetErrorString(e));
  e = grow(h, u.table, n);
  if (e == hipSuccess) e = grow(h, u.words, (long long)kRouteWords * n + 2LL * (levels + 1));
  if (e == hipSuccess) e = grow(h, u.sums, (long long)kRouteSums * n);
  if (e == hipSuccess) e = grow(h, u.h_offsets, (long long)levels + 1);
  if (e != hipSuccess) return wdpm_fail("wdpm_route_label: no memory for the routing of %lld ponds: %s", (long long)n, hipGetErrorString(e));
  u.timer.clear();
  u.levels = levels;
  u.plan = RoutePlan();
  if (n > 0) {
    const RouteArrays a = route_arrays(u.words.p, u.sums.p, n, levels);
    const dim3 grid(blocks_for(n, kBlock)), block(kBlock);
    HIP_TRY(hipMemsetAsync(a.offsets, 0, (size_t)(levels + 1) * sizeof(int), sm));
    HIP_TRY(u.timer.mark(h->timing, 0, sm));
    hipLaunchKernelGGL(route_init_kernel, grid, block, 0, sm, (long long)n, reinterpret_cast<const wdpm_pond *>(h->lab.table.p),
                       reinterpret_cast<const wdpm_pond_catchment *>(h->cat.table.p), reinterpret_cast<const wdpm_pond_outlet *>(h->out.table.p),
                       (const wdpm_pond_spill *)h->spl.table.p, a);
    hipLaunchKernelGGL(route_scan_kernel, dim3(1), block, 0, sm, levels, a);
    hipLaunchKernelGGL(route_scatter_kernel, grid, block, 0, sm, (long long)n, a);
    HIP_TRY(u.timer.mark(h->timing, 1, sm));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(u.h_offsets.p, a.offsets, (size_t)(levels + 1) * sizeof(int), hipMemcpyDeviceToHost, sm));
    if (wdpm_stream_sync(x, sm)) return 1;
    if (h->timing) HIP_TRY(u.timer.read(0, 1, &u.timer.ms[0]));
    const int *off = u.h_offsets.p;
    bool sound = off[0] == 0 && off[levels] == n;             /* every level of a chain holds a pond */
    for (int l = 0; sound && l < levels; l++) sound = off[l + 1] > off[l];
    if (!sound) return wdpm_fail("wdpm_route_label: the levels of %lld ponds do not add up", (long long)n);
    u.plan = route_plan(off, levels, u.narrow, u.run_levels);
  }
  if (route_sweep(h, n, runoff_q)) return 1;
  u.valid = true;
  h->lab.valid = true;
  if (nponds) *nponds = n;
  return 0;
}

extern "C" int wdpm_route_rerun(wdpm_ponds *h, double runoff_m) {
  if (!h) return wdpm_fail("wdpm_route_rerun: null handle");
  int64_t runoff_q = 0;
  if (check_runoff("wdpm_route_rerun", runoff_m, &runoff_q)) return 1;
  if (!h->lab.valid || !h->spl.valid || !h->rte.valid) return wdpm_fail("wdpm_route_rerun: %s", kNoTable);
  HIP_TRY(hipSetDevice(h->x->p.device));
  if (wdpm_synchronize(h->x)) return 1;                       /* behind everything the context has queued, as a read-out is */
  h->rte.valid = false;                                       /* a rerun that fails leaves no routing table */
  h->rte.timer.clear();
  if (route_sweep(h, h->lab.stats.ponds, runoff_q)) return 1;
  h->rte.valid = true;
  return 0;
}

extern "C" int wdpm_route_table(wdpm_ponds *h, wdpm_pond_route *out, int64_t capacity) {
  return table_out("wdpm_route_table", h, &wdpm_ponds::rte, kNoTable, out, capacity);
}

extern "C" int wdpm_route_stats(wdpm_ponds *h, wdpm_pond_route_stats *out) {
  return stats_out("wdpm_route_stats", h, &wdpm_ponds::rte, kNoTable, out);
}

extern "C" int wdpm_route_phase_ms(wdpm_ponds *h, double *ms) {
  return phase_ms_out("wdpm_route_phase_ms", h, &wdpm_ponds::rte, kNoTable, ms);
}
#endif  /* WDPM_PONDS_EMULATION */
