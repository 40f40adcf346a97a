/*
 * wdpm_block.hip — the block loop of include/wdpm.h on a context (wdpm_ctx.h): threshold flush and snapshot, the iterations of a
 * block as launches of the dispatch's choosing (wdpm_dispatch.h) - one by one, two per launch, replayed as HIP graphs or as three
 * overlapped windows - the folded max diff, and the timers that count all of it.
 * Replaces the reference's OpenCL host path (src/WDPMCL.c:598-638, :1126-1236).
 */
#include <cstring>

#include "wdpm_ctx.h"

/* chunk height of the iteration kernel once most tiles are dry (24 ... 384 rows measured in round 2: profiles/r02/sparse.txt) */
constexpr int kSparseChunkRows = 96;

/* What this context knows of an iteration launch over the window [A0, out_last] (wdpm_dispatch.h): `tiles` / `balanced` where the
 * launch comes with the context's dry-tile flags / balance state (whole-slab launches of wdpm_iterate). */
static LaunchRequest iteration_request(const wdpm_ctx *x, int A0, int out_last, int chunk_rows, bool max_diff, int leave_cus, const TilePlan *tiles,
                                       bool balanced) {
  LaunchRequest q{};
  q.module = x->p.module;
  q.g = x->g;
  q.A0 = A0;
  q.out_last = out_last;
  q.chunk_rows = chunk_rows;
  q.signed_zero_safe = x->negzero();
  q.flush = x->flush_pending;
  q.max_diff = max_diff;
  q.flags = launch_flags(x);
  q.leave_cus = leave_cus;
  q.codes32 = x->code.q != nullptr;
  q.codes16 = x->code.h != nullptr;
  q.force_codes = x->code.force;
  q.tiles_offered = tiles != nullptr;
  q.tile_capacity = tiles && tiles->zout ? tiles->capacity : 0;
  q.wide_tri_ok = tiles && tiles->wide_tri_ok;
  q.balance_mode = balanced ? x->bal.mode : 0;
  q.balance_capacity = x->bal.capacity;
  return q;
}

void drop_graphs(wdpm_ctx *x) {
  if (x->graphs.empty()) return;
  (void)hipStreamSynchronize(x->stream);             /* a replay may still be running */
  for (auto &ge : x->graphs) (void)hipGraphExecDestroy(ge.exec);
  x->graphs.clear();
}

/* the recorded pairs of every timer: their milliseconds to the timer, their events back to the pool.  A pair leaves its list as it
 * enters the pool, so that an error on the way leaves none in both. */
static int fold_timing(wdpm_ctx *x) {
  for (auto *t : x->timers())
    while (!t->pending.empty()) {
      const EventPair ep = t->pending.back();
      HIP_TRY(hipEventSynchronize(ep.b));
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, ep.a, ep.b));
      t->ms += ms;
      t->pending.pop_back();
      x->pool.push_back(ep);
    }
  return 0;
}

/* an event pair from the pool, or a new one */
static int take_pair(wdpm_ctx *x, EventPair *ep) {
  if (!x->pool.empty()) { *ep = x->pool.back(); x->pool.pop_back(); }
  else { HIP_TRY(hipEventCreate(&ep->a)); HIP_TRY(hipEventCreate(&ep->b)); }
  return 0;
}

/* the first event of a pair for timer `t`, recorded on the context's stream (a pending list grown long is folded first) */
static int start_pair(wdpm_ctx *x, const wdpm_ctx::Timer &t, EventPair *ep) {
  if (t.pending.size() >= 256 && fold_timing(x)) return 1;
  if (take_pair(x, ep)) return 1;
  HIP_TRY(hipEventRecord(ep->a, x->stream));
  return 0;
}

static int timing_get(wdpm_ctx *x, const wdpm_ctx::Timer &t, int64_t *count, double *ms) {
  if (bind(x)) return 1;
  if (fold_timing(x)) return 1;
  if (count) *count = t.count;
  if (ms) *ms = t.ms;
  return 0;
}

static int one_pass(wdpm_ctx *x, int oi, int oj) {
  if (ensure_private(x)) return 1;
  x->zero_valid[x->cur] = false;
  HIP_TRY(wdpm_launch_pass(x->p.module, x->d_w[x->cur], x->d_dem, x->g, oi, oj, x->d_scal, x->stream));
  return 0;
}

/* what a call of wdpm_iterate decides before its first launch */
struct IterateCall {
  int n_iter;
  bool fold;        /* the last launch folds the max diff the caller announced (wdpm_expect_max_diff) */
  bool steady;      /* the launches between the first and the last are timed by `st`, the whole call by `ep` where timing is on */
  EventPair ep, st;
};

static int begin_call(wdpm_ctx *x, int n_iter, IterateCall *call) {
  *call = IterateCall{n_iter, x->md_hint && x->kernel == WDPM_KERNEL_FUSED && x->p.module != WDPM_DRAIN && !x->negzero(),
                      x->timing && n_iter >= 3 && x->kernel == WDPM_KERNEL_FUSED, {nullptr, nullptr}, {nullptr, nullptr}};
  x->md_hint = x->md_valid = false;
  /* stencil timing is opt-in (wdpm_timing_reset switches it on): two event records per call are a
   * measurable share of a small raster's iteration */
  if (x->timing && start_pair(x, x->t_call, &call->ep)) return 1;
  return call->steady ? take_pair(x, &call->st) : 0;
}

static int end_call(wdpm_ctx *x, const IterateCall &call) {
  if (x->timing) {
    HIP_TRY(hipEventRecord(call.ep.b, x->stream));
    x->t_call.pending.push_back(call.ep);
  }
  if (call.steady) {
    x->t_steady.pending.push_back(call.st);
    x->t_steady.count += call.n_iter - 2;
  }
  return 0;
}

/* whether a whole-slab launch of this context keeps the dry-tile flags, and its chunk height (0: the planner's) */
struct SlabPolicy { bool track; int chunk_rows; };
static SlabPolicy whole_slab_policy(const wdpm_ctx *x) {
  /* A mostly wet raster (the last block that kept flags found most tiles working) drops the dry-tile flags for chunk heights
   * that follow the XCDs' speeds (wdpm_kernels.h::XcdBalance): a tiling of its own.  The flags are looked at again every 16 blocks. */
  const bool balanced = x->bal.mode == 2 || (x->bal.mode == 1 && x->wide_tri_ok);
  const bool track = x->tiles_mode != 0 && !x->negzero() && !balanced;
  /* sparse rasters march short chunks: the launch takes as long as its wettest tile */
  return {track, x->p.chunk_rows >= 3 ? x->p.chunk_rows : (track && x->sparse ? kSparseChunkRows : 0)};
}

/* what a launch that may reduce max |w - oldw| over the rows the caller announced is given; with `fold` it does, into a cell zeroed here */
static int max_diff_args(wdpm_ctx *x, bool fold, MaxDiffArgs *md) {
  *md = MaxDiffArgs{fold ? x->d_w[x->old] : nullptr, x->flush_thres, x->md_lo, x->md_hi, x->d_md};
  if (fold) HIP_TRY(hipMemsetAsync(x->d_md, 0, sizeof(unsigned long long), x->stream));
  return 0;
}

/* The host's state after an iteration launch that read d_w[cur] whole and wrote d_w[t], `advanced` iterations on; `tp`: the tile
 * plan of a launch that maintained t's dry-tile flags, else nullptr. */
static int launched(wdpm_ctx *x, int t, int advanced, const TilePlan *tp) {
  if (x->flush_pending) flushed_whole(x, x->flush_thres);   /* the launch flushed every value it loaded, and it loaded them all */
  if (tp) {
    if (tp->nstrips != x->tile_nstrips || tp->H != x->tile_H || tp->nchunks != x->tile_nchunks) {
      /* another tiling from here on: nothing known about any raster, and the flag arrays get their border of
       * 1s for the new pitch (queued behind the launch, which wrote t's interior flags: only the other two) */
      x->zero_valid[0] = x->zero_valid[1] = x->zero_valid[2] = false;
      x->tile_nstrips = tp->nstrips; x->tile_H = tp->H; x->tile_nchunks = tp->nchunks;
      for (int i = 0; i < 3; i++)
        if (i != t) HIP_TRY(hipMemsetAsync(x->d_zero[i], 1, (size_t)x->tile_cap, x->stream));
    }
    x->tiles_launched += (int64_t)tp->nstrips * tp->nchunks;
  }
  x->zero_valid[t] = tp != nullptr;
  x->cur = t;
  x->flush_pending = false;
  x->drain_owed = x->p.module == WDPM_DRAIN;     /* this iteration's drain(): owed to the next launch or reader */
  x->t_call.count += advanced;
  return 0;
}

/* One launch of the fused kernels over the whole slab, as iteration `it` of the call.  *did: iterations it advanced the raster by -
 * two where the dispatch offers both in one launch (plan_iter2); did == nullptr: one, never two (launches before and inside a graph) */
static int fused_step(wdpm_ctx *x, const IterateCall &call, const int it, int *did) {
  if (call.steady && it == 1) HIP_TRY(hipEventRecord(call.st.a, x->stream));
  if (call.steady && it == call.n_iter - 1) HIP_TRY(hipEventRecord(call.st.b, x->stream));
  if (x->flush_pending && x->negzero() && wdpm_apply_owed_flush(x)) return 1;   /* no flush-on-load variant of that kernel */
  const int t = free_slot(x);
  TilePlan tp{x->d_zero[x->cur], x->d_zero[t], x->zero_valid[x->cur] ? 1 : 0, x->zero_valid[t] ? 1 : 0, x->d_active,
              x->tile_cap, x->tile_nstrips, x->tile_H, x->tile_nchunks, 0, x->wide_tri_ok ? 1 : 0};
  const SlabPolicy pol = whole_slab_policy(x);
  /* the block's last iteration also reduces max |w - oldw| over the rows the caller announced */
  MaxDiffArgs md;
  if (max_diff_args(x, call.fold && it == call.n_iter - 1, &md)) return 1;
  const LaunchRequest q = iteration_request(x, 0, x->g.rows - 1, pol.chunk_rows, md.old != nullptr, 0, pol.track ? &tp : nullptr, x->bal.mode != 0);
  const IterationBuffers buf{x->d_w[x->cur], x->d_w[t], x->d_dem, &x->code, x->flush_pending ? x->flush_thres : 0.0, x->drain_owed ? 1 : 0,
                             x->d_scal, x->stream, pol.track ? &tp : nullptr, &md, &x->bal, x->d_iter2_err};
  /* iterations from this one on that are launches like it: not the block's last where that folds the max diff - and, where the
   * steady launches are timed, neither the call's first nor its last */
  int alike = 0;
  if (did && !x->flush_pending && !md.old && !(call.steady && it == 0))
    alike = call.n_iter - it - ((call.fold || call.steady) ? 1 : 0);
  const LaunchPlan plan = alike >= 2 ? plan_iter2(q, *x->facts, wdpm_switches(), alike) : plan_iteration(q, *x->facts, wdpm_switches());
  const int advanced = plan.iter2 ? 2 : 1;
  if (did) *did = advanced;
  HIP_TRY(wdpm_launch_iteration(q, plan, buf));
  if (md.old) x->md_valid = true;
  return launched(x, t, advanced, pol.track && tp.maintained ? &tp : nullptr);
}

/* one iteration as the pass kernel's nine colour passes, each a launch, and the drain module's drain() */
static int pass_step(wdpm_ctx *x) {
  for (int oi = 1; oi <= 3; oi++)
    for (int oj = 1; oj <= 3; oj++)
      if (one_pass(x, oi, oj)) return 1;
  x->t_call.count += 9;
  if (x->p.module == WDPM_DRAIN)
    HIP_TRY(wdpm_launch_drain_outlet(x->d_w[x->cur], x->d_dem, x->g, x->d_scal, x->stream));
  return 0;
}

/* Small rasters are launch-bound (482 x 471: 5.2 us of kernel, 6.3 us from launch to launch when the host queues them one by one):
 * the iterations between a block's first (threshold flush on load) and last (max diff) are replayed as HIP graphs of kGraphIters
 * launches each, captured from wdpm_iterate's own steps (round 5; `tools/graph_probe.py` measured +21 % for add at that size, +3 % for
 * drain, nothing from 2048^2 up).  Only where a launch keeps no state on the host (the relay / triangle kernels: no tile flags, no
 * balance table) and nobody times the launches; the rasters ping-pong between two buffers within a block, so an even count returns
 * to the state it was captured in.  WDPM_GRAPH=0: never. */
constexpr int kGraphIters = 32;

static bool graphs_apply(wdpm_ctx *x, const IterateCall &call) {
  if (x->kernel != WDPM_KERNEL_FUSED || x->timing || call.n_iter < kGraphIters + 2 || x->graph_mode == 0) return false;
  if (x->graph_mode < 0) { const char *e = getenv("WDPM_GRAPH"); x->graph_mode = (e && atoi(e) == 0) ? 0 : 1; }
  const SlabPolicy pol = whole_slab_policy(x);
  TilePlan tq{nullptr, nullptr, 0, 0, nullptr, 0, 0, 0, 0, 0, x->wide_tri_ok ? 1 : 0};
  /* would a whole-slab steady launch (no flush, no folded max diff) of this context go to the relay / triangle kernels of small
   * rasters?  Asks the dispatch itself. */
  LaunchRequest steady = iteration_request(x, 0, x->g.rows - 1, pol.chunk_rows, false, 0, pol.track ? &tq : nullptr, false);
  steady.flush = false;
  const LaunchPlan sp = plan_iteration(steady, *x->facts, wdpm_switches());
  return x->graph_mode == 1 && !sp.error && sp.family != WDPM_FAMILY_MARCHING;
}

/* iterations *it ... of the call, kGraphIters at a time, while that leaves the call its last launch */
static int replay_steady(wdpm_ctx *x, const IterateCall &call, int *it) {
  while (call.n_iter - 1 - *it >= kGraphIters && x->graph_mode == 1) {
    const wdpm_ctx::GraphKey key{x->code.q, x->code.h, x->cur, x->old, launch_flags(x), x->drain_owed ? 1 : 0, whole_slab_policy(x).chunk_rows,
                                 x->g.dr, x->g.dc, x->wide_tri_ok ? 1 : 0, x->code.force, x->kinds};
    hipGraphExec_t exec = nullptr;
    for (const auto &ge : x->graphs)
      if (!memcmp(&ge.key, &key, sizeof key)) { exec = ge.exec; break; }
    if (!exec) {
      /* capture kGraphIters launches of wdpm_iterate's (nothing runs yet; the host's bookkeeping moves on as if they had) */
      hipGraph_t graph = nullptr;
      if (hipStreamBeginCapture(x->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); x->graph_mode = 0; break; }
      int bad = 0;
      for (int k = 0; k < kGraphIters && !bad; k++) bad = fused_step(x, call, *it + k, nullptr);
      const hipError_t ec = hipStreamEndCapture(x->stream, &graph);
      if (bad || ec != hipSuccess || !graph || hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        x->graph_mode = 0;
        return wdpm_fail("wdpm_iterate: capturing %d iterations as a HIP graph failed (set WDPM_GRAPH=0 to launch them one by one)", kGraphIters);
      }
      (void)hipGraphDestroy(graph);
      if (x->graphs.size() >= 12) drop_graphs(x);
      x->graphs.push_back({key, exec});
    } else {
      /* what kGraphIters steps leave on the host: the same current raster (an even count), nothing known about dry tiles of the
       * two rasters written, drain() owed by the last launch */
      for (int k = 0; k < kGraphIters; k++)
        if (launched(x, free_slot(x), 1, nullptr)) return 1;
    }
    HIP_TRY(hipGraphLaunch(exec, x->stream));
    x->graph_launches++;
    *it += kGraphIters;
  }
  return 0;
}

extern "C" {

int wdpm_begin_block(wdpm_ctx *x, double thres) {
  if (bind(x)) return 1;
  x->md_valid = x->md_hint = false;
  if (wdpm_apply_owed_flush(x)) return 1;                /* a flush still owed from a block that never iterated */
  if (x->kernel == WDPM_KERNEL_FUSED && !x->negzero()) {
    /* no pass over the raster: the current raster becomes the snapshot, the flush rides on the next launch's loads */
    x->old = x->cur;
    x->flush_pending = true;
  } else {
    const int t = x->cur == x->old ? free_slot(x) : x->old;
    HIP_TRY(wdpm_launch_flush_snapshot(x->d_w[x->cur], x->d_w[t], x->cells, thres, x->stream));
    x->zero_valid[t] = false;
    x->old = t;
    flushed_whole(x, thres);
  }
  x->flush_thres = thres;
  HIP_TRY(hipMemcpyAsync(x->d_scal + 1, x->d_scal, sizeof(double), hipMemcpyDeviceToDevice, x->stream)); /* olddrain */
  return 0;
}

int wdpm_xch_timing_begin(wdpm_ctx *x, EventPair *ep) {
  ep->a = ep->b = nullptr;
  return x->timing ? start_pair(x, x->t_xch, ep) : 0;
}

int wdpm_xch_timing_end(wdpm_ctx *x, const EventPair *ep) {
  if (!ep->a) return 0;
  HIP_TRY(hipEventRecord(ep->b, x->stream));
  x->t_xch.pending.push_back(*ep);
  x->t_xch.count += 1;
  return 0;
}

int wdpm_pass(wdpm_ctx *x, int32_t oi, int32_t oj) {
  if (oi < 1 || oi > 3 || oj < 1 || oj > 3) return wdpm_fail("wdpm_pass: oi,oj must be in 1..3");
  if (bind(x)) return 1;
  return one_pass(x, oi, oj);
}

int wdpm_drain_outlet(wdpm_ctx *x) {
  if (x->p.module != WDPM_DRAIN) return 0;
  if (bind(x) || ensure_private(x)) return 1;
  HIP_TRY(wdpm_launch_drain_outlet(x->d_w[x->cur], x->d_dem, x->g, x->d_scal, x->stream));
  return 0;
}

int wdpm_iterate(wdpm_ctx *x, int32_t n_iter) {
  if (n_iter < 0) return wdpm_fail("wdpm_iterate: negative iteration count");
  if (n_iter == 0) return 0;
  if (bind(x)) return 1;
  IterateCall call;
  if (begin_call(x, n_iter, &call)) return 1;
  int it = 0;
  if (graphs_apply(x, call)) {
    if (fused_step(x, call, it++, nullptr)) return 1;      /* the block's first launch: as ever */
    if (replay_steady(x, call, &it)) return 1;
  }
  while (it < n_iter) {
    int did = 1;
    if (x->kernel == WDPM_KERNEL_FUSED ? fused_step(x, call, it, &did) : pass_step(x)) return 1;
    it += did;
  }
  return end_call(x, call);
}

int wdpm_iterate_overlapped(wdpm_ctx *x, int32_t n_iter, int32_t top_rows, int32_t bottom_rows) {
  if (n_iter < 0 || top_rows < 0 || bottom_rows < 0) return wdpm_fail("wdpm_iterate_overlapped: negative argument");
  const int rows = x->g.rows;
  /* window boundaries: the top launch produces rows [0, t_last] with (t_last + 1) % 3 == 2, the bottom
   * launch rows [b_first, rows-1] with b_first % 3 == 2, the interior launch the rows between */
  int t_last = -1, b_first = rows;
  if (top_rows > 0) { t_last = top_rows - 1; while ((t_last + 1) % 3 != 2) t_last++; }
  if (bottom_rows > 0) { b_first = rows - bottom_rows; while (b_first % 3 != 2) b_first--; }
  const bool usable = x->kernel == WDPM_KERNEL_FUSED && x->p.module != WDPM_DRAIN && n_iter > 0 &&
                      (top_rows > 0 || bottom_rows > 0) && b_first - (t_last + 1) >= 24 && t_last < rows - 1 &&
                      b_first >= 2;
  if (!usable) return wdpm_iterate(x, n_iter);
  const bool hint = x->md_hint;
  x->md_hint = false;
  if (n_iter > 1 && wdpm_iterate(x, n_iter - 1)) return 1;
  x->md_hint = hint;
  if (bind(x)) return 1;
  if (x->flush_pending && x->negzero() && wdpm_apply_owed_flush(x)) return 1;
  const int t_slot = free_slot(x);
  const double *w_in = x->d_w[x->cur];
  double *w_out = x->d_w[t_slot];
  const bool fold = x->md_hint && !x->negzero();     /* (usable: fused kernel, not the drain module) */
  x->md_hint = x->md_valid = false;
  MaxDiffArgs md;
  if (max_diff_args(x, fold, &md)) return 1;
  /* stencil timing of this iteration: from here on the main stream to the end of the interior launch
   * on the side stream (the longest of the three) */
  EventPair ep{nullptr, nullptr};
  if (x->timing && start_pair(x, x->t_call, &ep)) return 1;
  HIP_TRY(hipEventRecord(x->ev_fork, x->stream));               /* w_in is complete here */
  /* one window of the three: no tile flags (not the tiling they are kept for), no balance table */
  auto window = [&](const int A0, const int out_last, const int leave_cus, hipStream_t s) -> hipError_t {
    const LaunchRequest q = iteration_request(x, A0, out_last, x->p.chunk_rows, fold, leave_cus, nullptr, false);
    const IterationBuffers buf{w_in, w_out, x->d_dem, &x->code, x->flush_pending ? x->flush_thres : 0.0, 0, x->d_scal, s, nullptr, &md, nullptr};
    return wdpm_launch_iteration(q, plan_iteration(q, *x->facts, wdpm_switches()), buf);
  };
  if (t_last >= 0) HIP_TRY(window(0, t_last, 0, x->stream));
  if (b_first < rows) HIP_TRY(window(b_first - 2, rows - 1, 0, x->stream));
  HIP_TRY(hipStreamWaitEvent(x->side, x->ev_fork, 0));
  /* 8 of 256 CUs stay free for the RCCL kernels of the refresh that follows */
  HIP_TRY(window(t_last >= 0 ? t_last - 1 : 0, b_first < rows ? b_first - 1 : rows - 1, x->comm ? 8 : 0, x->side));
  if (x->timing) {
    HIP_TRY(hipEventRecord(ep.b, x->side));
    x->t_call.pending.push_back(ep);
  }
  HIP_TRY(hipEventRecord(x->ev_join, x->side));
  x->pending_join = true;
  if (fold) x->md_valid = true;
  x->t_call.count += 3;
  return launched(x, t_slot, 0, nullptr);   /* no flags kept: three windows, not the tiling they are for; the launches are counted above */
}

int wdpm_expect_max_diff(wdpm_ctx *x, int32_t row_lo, int32_t row_hi) {
  if (!rows_inside(x, row_lo, row_hi)) return wdpm_fail("wdpm_expect_max_diff: bad row range");
  /* a result already folded by the last launch stays good for ITS rows only (an expectation for other rows, with no
   * iteration after it, must not be answered from it: tests/test_hip_parity.py::test_random_call_sequences) */
  if (x->md_valid && (x->md_lo != row_lo || x->md_hi != row_hi)) x->md_valid = false;
  x->md_hint = true;
  x->md_lo = row_lo;
  x->md_hi = row_hi;
  return 0;
}

int wdpm_max_diff(wdpm_ctx *x, int32_t row_lo, int32_t row_hi, double *out) {
  if (!rows_inside(x, row_lo, row_hi) || !out) return wdpm_fail("wdpm_max_diff: bad row range");
  if (bind(x)) return 1;
  if (wdpm_apply_owed_flush(x)) return 1;
  const bool folded = x->md_valid && x->md_lo == row_lo && x->md_hi == row_hi;   /* the last iteration launch already reduced it */
  /* the snapshot may hold the raster as it was BEFORE the block's flush: the kernel applies the flush as it reads */
  if (folded) HIP_TRY(hipMemcpyAsync(x->d_bits, x->d_md, sizeof(unsigned long long), hipMemcpyDeviceToDevice, x->stream));
  else HIP_TRY(wdpm_launch_max_diff(x->d_w[x->cur], x->d_w[x->old], x->flush_thres, x->d_dem, x->g, row_lo, row_hi, x->d_bits, x->stream));
  HIP_TRY(hipMemcpyAsync(x->h_pin, x->d_bits, sizeof(double), hipMemcpyDeviceToHost, x->stream));
  const bool look = x->tiles_launched > 0;
  if (look) {
    HIP_TRY(hipMemcpyAsync(x->h_active, x->d_active, sizeof(unsigned), hipMemcpyDeviceToHost, x->stream));
    HIP_TRY(hipMemsetAsync(x->d_active, 0, sizeof(unsigned), x->stream));
  }
  if (wdpm_stream_sync(x, x->stream)) return 1;
  *out = x->h_pin[0];
  if (look) {
    /* once per block: how many tiles worked?  Mostly dry -> short chunks from the next block on (and back) */
    const double frac = (double)*x->h_active / (double)x->tiles_launched;
    x->stat_tiles += x->tiles_launched;
    x->stat_active += *x->h_active;
    x->tiles_launched = 0;
    if (!x->sparse && frac < 0.30 && x->g.rows >= 4 * kSparseChunkRows) x->sparse = true;
    else if (x->sparse && frac > 0.60) x->sparse = false;
    /* mostly wet: a raster of a few rounds of triangle waves goes to that kernel from the next block on (no flags there, so
     * the marching kernel looks again every 16 blocks) */
    x->wide_tri_ok = !x->sparse && frac > 0.60;
    x->blocks_unprobed = 0;
  } else if (x->wide_tri_ok && ++x->blocks_unprobed >= 16) {
    x->wide_tri_ok = false;
  }
  return 0;
}

int wdpm_run_block(wdpm_ctx *x, int32_t n_iter, double thres, double *max_diff) {
  if (wdpm_begin_block(x, thres)) return 1;
  if (wdpm_expect_max_diff(x, 0, x->g.rows)) return 1;
  if (wdpm_iterate(x, n_iter)) return 1;
  return wdpm_max_diff(x, 0, x->g.rows, max_diff);
}

int wdpm_timing_reset(wdpm_ctx *x) {
  if (bind(x)) return 1;
  if (fold_timing(x)) return 1;
  for (auto *t : x->timers()) { t->count = 0; t->ms = 0.0; }
  x->timing = true;
  return 0;
}

int wdpm_timing_get_exchange(wdpm_ctx *x, int64_t *refreshes, double *ms) { return timing_get(x, x->t_xch, refreshes, ms); }
int wdpm_timing_get_steady(wdpm_ctx *x, int64_t *launches, double *ms) { return timing_get(x, x->t_steady, launches, ms); }
int wdpm_timing_get(wdpm_ctx *x, int64_t *launches, double *ms) { return timing_get(x, x->t_call, launches, ms); }

int wdpm_balance_info(wdpm_ctx *x, int32_t *updates, double *weights9) {
  if (updates) *updates = x->bal.mode ? x->bal.updates : 0;
  if (!weights9) return 0;
  for (int i = 0; i < 9; i++) weights9[i] = i < 8 ? 1.0 : 0.95;
  if (!x->bal.mode || !x->bal.weight) return 0;
  if (bind(x)) return 1;
  float w[9];
  HIP_TRY(hipMemcpyAsync(w, x->bal.weight, sizeof w, hipMemcpyDeviceToHost, x->stream));
  if (wdpm_stream_sync(x, x->stream)) return 1;
  for (int i = 0; i < 9; i++) weights9[i] = (double)w[i];
  return 0;
}

} /* extern "C" */
