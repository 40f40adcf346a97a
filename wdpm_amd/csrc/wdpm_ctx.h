/*
 * wdpm_ctx.h — the context object behind the opaque wdpm_ctx of include/wdpm.h (HIP back-end), and what the units that work on it
 * share.  Internal to the product library: wdpm_capi.hip (life cycle, data movement, options), wdpm_block.hip (block loop),
 * wdpm_dem_codes.hip (DEM codes), wdpm_stats.hip (statistics), wdpm_rccl.hip (RCCL halos) and the pond units.
 */
#ifndef WDPM_CTX_H
#define WDPM_CTX_H

#include <hip/hip_runtime.h>

#include <array>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "../../include/wdpm.h"
#include "wdpm_kernels.h"

struct wdpm_comm;   /* RCCL communicator state of a context (wdpm_rccl.hip) */

struct EventPair { hipEvent_t a, b; };

constexpr DemCode kNoCodes = DemCode{nullptr, 0.0, 1.0, 1.0, 0.0, 0, nullptr, nullptr, 0};   /* the fp64 DEM is in charge */
/* Spare cells behind the DEM and each water raster: the fused kernel's dump area for masked-out stores (a strip's width), and what an
 * edge wave's three-column loads may read past the end of the slab's last row (two cells; the DEM codes have spare cells too) */
constexpr size_t kRasterSpare = 192 * sizeof(double);
constexpr int dem_groups(int ncp) { return (ncp + kDemGroup - 1) / kDemGroup; }   /* DemCode::ngroups of a row of ncp columns */

/* Every member initialises itself: wdpm_create sets only what depends on its parameters or on the environment. */
struct wdpm_ctx {
  wdpm_params p{};
  const DeviceFacts *facts = nullptr;   /* of p.device, for the launch planner (wdpm_dispatch.h) */
  SlabGeom g{};
  size_t cells = 0;
  hipStream_t stream = nullptr;
  bool own_stream = true;
  double *d_dem = nullptr, *d_w[3] = {};   /* three water rasters: the current one, the iteration kernel's write target, the snapshot */
  int cur = 0;                  /* d_w[cur] is bigwater */
  int old = 2;                  /* d_w[old] is oldwater (WDPMCL.c:1069-1073) - possibly still UNFLUSHED, see flush_pending */
  bool flush_pending = false;   /* wdpm_begin_block's threshold flush has not been applied yet: cur == old, and the next
                                   iteration launch applies it while loading (no pass over the raster of its own) */
  /* dry-tile skipping (wdpm_kernels.h::TileFlags): one flag array per water raster, valid for one tiling */
  unsigned char *d_zero[3] = {};
  bool zero_valid[3] = {};      /* d_zero[i] describes d_w[i]'s current content (for tiling tile_*) */
  int tile_cap = 0, tile_nstrips = 0, tile_H = 0, tile_nchunks = 0;
  unsigned *d_active = nullptr; /* waves that did not skip since the last look */
  unsigned *h_active = nullptr; /* pinned */
  int64_t tiles_launched = 0;   /* tiles of the flag-maintaining launches since the last look */
  bool sparse = false;          /* most tiles are dry: short chunks (96 rows), so that a wet tile is a short march */
  bool wide_tri_ok = false;     /* the last block that kept tile flags found > 60 % of the tiles working: mid-size rasters may go to the
                                 * triangle kernel (no flags); probed again with the marching kernel every 16 blocks */
  int blocks_unprobed = 0;
  int tiles_mode = 1;           /* 1 on (default), 0 off (WDPM_TILES=0 / WDPM_OPT_TILES) */
  int64_t stat_tiles = 0, stat_active = 0;   /* running totals for wdpm_get_option */
  /* max |w - oldw| folded into the last iteration launch of a block (wdpm_expect_max_diff) */
  unsigned long long *d_md = nullptr;   /* its reduction cell */
  bool md_hint = false, md_valid = false;   /* the next wdpm_iterate may fold it / d_md holds the value for rows [md_lo, md_hi) */
  int md_lo = 0, md_hi = 0;
  bool drain_owed = false;      /* drain module: the last iteration's drain() (WDPMCL.c:1089) has not been applied to d_w[cur];
                                   the next iteration launch does it as it loads, anybody else asks wdpm_apply_owed_drain() first */
  double flush_thres = -__builtin_inf();   /* the threshold of the current block: the flush still owed to d_w[cur] (flush_pending)
                                   and to the snapshot when wdpm_max_diff reads it; -inf = none */
  double *d_scal = nullptr;             /* [0] totaldrain, [1] olddrain */
  unsigned long long *d_bits = nullptr; /* max-diff reduction cell; three words for wdpm_launch_dem_min */
  double *h_pin = nullptr;              /* pinned staging: 4 doubles (read_back) */
  unsigned *h_iter2_err = nullptr;      /* pinned, and written by the device: Iter2Args::err (looked at wherever the host waits for the stream) */
  unsigned *d_iter2_err = nullptr;      /* the same word as the device sees it */
  unsigned long long *d_stat = nullptr; /* wdpm_count_stats / wdpm_find_drain: 4 reduction cells */
  double *d_sum_approx = nullptr;       /* wdpm_volume_partial: per-chunk approximate sums, integer sums, binades, flags */
  long long *d_sum_i = nullptr;
  int *d_sum_k = nullptr;
  unsigned *d_sum_flag = nullptr;
  int kernel = 0;               /* resolved WDPM_KERNEL_* */
  /* What the current raster may hold, as WDPM_WATER_* bits (wdpm_kernels.h::wdpm_launch_scan_water): NEGZERO a -0.0 depth was uploaded
   * (or the caller asked) - the exact-zero stencil variant; NEGATIVE negative depths (until the next threshold flush with thres >= 0);
   * ODD NaN, absurd depths or water on NODATA cells (for good).  With none of them the gate-free kernel variants run
   * (wdpm_iteration.h: PLAIN).  Nothing is known before the first upload. */
  unsigned kinds = WDPM_WATER_ODD;
  bool negzero() const { return (kinds & WDPM_WATER_NEGZERO) != 0; }
  bool plain() const { return kinds == 0; }
  struct GuardedBuffer { char *base; size_t bytes; };   /* base = start of the front guard band; bytes = payload between the bands */
  std::vector<GuardedBuffer> guards;   /* WDPM_GUARD_KB: the buffers wdpm_get_option(WDPM_OPT_GUARD_BAD) inspects */
  int *d_dem32 = nullptr;       /* the DEM as verified-lossless 32-bit codes (wdpm_kernels.h::DemCode) */
  DemCode code = kNoCodes;      /* code.q == d_dem32 while the uploaded DEM is encodable and the option is on */
  bool dem32_encodable = false;
  int dem_grid = 0, dem_grid_exp = 0;   /* what upload found: D = dem_grid ^ dem_grid_exp (10^e or 2^s), 0 / 0 while the fp64 DEM is in charge (WDPM_OPT_DEM_GRID, _EXP) */
  unsigned short *d_dem16 = nullptr;    /* the codes once more as 16-bit offsets from d_gbase (DemCode::h, ::gb); code.h is set while they are in use */
  int *d_gbase = nullptr;
  bool dem16_encodable = false;
  bool dem16_wanted = true;     /* WDPM_OPT_DEM16 as last set (default on); what runs is decided with dem16_encodable and code.q */
  XcdBalance bal{};             /* chunk heights by what each XCD delivers (wdpm_kernels.h); bal.mode == 0: off */
  bool dem_bounded = false;     /* every valid elevation of the uploaded DEM is below 2^30 m in magnitude (scan_dem): the clamped
                                   neighbour step may run where the depths allow it (wdpm_kernels.h: WDPM_LAUNCH_CLAMP_OK) */
  /* wdpm_iterate_overlapped: side stream for the interior launch and the event that joins it */
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool pending_join = false;
  hipEvent_t ev_copy[2] = {};   /* wdpm_copy_rows: [0] "my rows are produced" as source, [1] "the copy has read them" as destination */
  /* HIP graphs of steady small-raster iterations (wdpm_block.hip: wdpm_iterate).  A launch of the relay / triangle kernels keeps no state
   * on the host, and within a block the water rasters ping-pong between two buffers: an even number of iterations captured once from
   * the context's own launches replays any number of times from the same pair.  What a captured launch was given is the key, what the
   * water held (`kinds`) included: compared with memcmp, so it has no padding bytes and a field added to it is compared without further ado. */
  struct GraphKey {
    const void *q, *h;
    int cur, old, flags, drain_owed, chunk_rows, dr, dc, wide, force;
    unsigned kinds;
  };
  static_assert(std::has_unique_object_representations_v<GraphKey>, "GraphKey is compared with memcmp: no padding");
  struct GraphEntry { GraphKey key; hipGraphExec_t exec; };
  std::vector<GraphEntry> graphs;
  int graph_mode = -1;          /* -1 unknown, 0 off (WDPM_GRAPH=0, or a capture failed on this context), 1 on */
  int64_t graph_launches = 0;   /* graphs launched so far (WDPM_OPT_GRAPH_LAUNCHES) */
  /* stencil timing, three kinds of it: what was counted, the event pairs recorded and not yet read, the milliseconds of those that
   * were (fold_timing); the events of a pair that was read wait in `pool` for their next use */
  struct Timer { int64_t count = 0; double ms = 0.0; std::vector<EventPair> pending; };
  Timer t_call;                 /* whole calls of wdpm_iterate; count: an iteration of the fused kernels 1, of the pass kernel 9, an overlapped one 3 */
  /* the same for the launches of a call between its first and its last (those two may be the flush-on-load and the
   * max-diff variants of the kernel): what rocprofv3 lists as the dominant kernel */
  Timer t_steady;
  /* halo refreshes (wdpm_comm_exchange, wdpm_copy_rows into this context): from the point of the stream where the transfer is
   * queued to the point where the rows have arrived - what an N-GPU bench line needs to explain its scaling */
  Timer t_xch;
  std::array<Timer *, 3> timers() { return {&t_call, &t_steady, &t_xch}; }
  std::vector<EventPair> pool;
  bool timing = false;          /* record the event pairs at all (off until wdpm_timing_reset asks) */
  wdpm_comm *comm = nullptr;    /* wdpm_comm_init_rank / wdpm_comm_init_all, or nullptr */
  bool leak = false;            /* a guarded RCCL call or a stream wait ran past its deadline: somebody may still be using this
                                   context's stream and buffers, so wdpm_destroy frees none of them */
};

/* sets wdpm_last_error() of the calling thread and returns 1 */
int wdpm_fail(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return wdpm_fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

void wdpm_comm_release(wdpm_ctx *x);   /* wdpm_destroy's hook */
/* hipStreamSynchronize - with a deadline when the context has a communicator (a transfer whose peer has died never completes):
 * WDPM_SYNC_TIMEOUT_S, default 600 s; past it the communicator is aborted, the context is marked `leak` and 1 is returned */
int wdpm_stream_sync(wdpm_ctx *x, hipStream_t s);
/* halo-refresh timing (only while wdpm_timing_reset has switched timing on): begin records an event on the context's stream and
 * returns the pair, end records its second event */
extern "C" int wdpm_xch_timing_begin(wdpm_ctx *x, EventPair *ep);
extern "C" int wdpm_xch_timing_end(wdpm_ctx *x, const EventPair *ep);

/* ---- what the units share; every one returns 0, or 1 with wdpm_last_error() set ---- */
/* the context's device is current, and the interior launch of the last overlapped iteration is ordered before anything queued from here on */
inline int bind(wdpm_ctx *x) {
  HIP_TRY(hipSetDevice(x->p.device));
  if (x->pending_join) {
    HIP_TRY(hipStreamWaitEvent(x->stream, x->ev_join, 0));
    x->pending_join = false;
  }
  return 0;
}
inline int free_slot(const wdpm_ctx *x) {            /* a raster that is neither current nor the snapshot */
  for (int i = 0; i < 3; i++)
    if (i != x->cur && i != x->old) return i;
  return 0;
}
inline bool rows_inside(const wdpm_ctx *x, int lo, int hi) { return lo >= 0 && hi <= x->g.rows && lo <= hi; }   /* rows [lo, hi) lie in the slab */
/* the block's threshold flush has just been applied to the whole current raster: with thres >= 0 no negative depth is left */
inline void flushed_whole(wdpm_ctx *x, double thres) {
  if (thres >= 0.0) x->kinds &= ~(unsigned)WDPM_WATER_NEGATIVE;
}
/* the switches of the iteration dispatch (wdpm_dispatch.h): read from the environment once per process */
inline const Switches &wdpm_switches() {
  static const Switches sw = wdpm_read_switches(getenv);      /* (initialised under the compiler's lock: rank threads launch concurrently) */
  return sw;
}
/* wdpm_dispatch.h: WDPM_LAUNCH_PLAIN | WDPM_LAUNCH_CLAMP_OK for the iteration launches of this context */
inline int launch_flags(const wdpm_ctx *x) { return wdpm_launch_flags(wdpm_switches(), x->plain(), x->dem_bounded); }
/* rows [row, row + nrows) of the current raster are about to be (or have been) written by somebody other than the iteration kernel:
 * the tiles they touch are no longer known to be dry, a folded max diff over them no longer holds */
int wdpm_tiles_touch(wdpm_ctx *x, int row, int nrows);
/* readers of d_w[cur] or of totaldrain - drain module: the last iteration's drain() is applied if it has not been (before rows leave the context) */
int wdpm_apply_owed_drain(wdpm_ctx *x);
/* readers of d_w[cur]: that, and the block's threshold flush is applied in place if the current raster is still owed it */
int wdpm_apply_owed_flush(wdpm_ctx *x);
/* in-place writers of d_w[cur]: drained, flushed, and no longer the snapshot's buffer (a copy where it was) */
int ensure_private(wdpm_ctx *x);
/* a whole new raster is about to be written: d_w[cur] is a buffer other than the snapshot's, nothing known about its tiles */
int ensure_fresh_slot(wdpm_ctx *x);
/* no captured launch survives: they carry what they were given by value (GraphKey) - a new DEM, other codes or another outlet end them */
void drop_graphs(wdpm_ctx *x);
/* the DEM just uploaded as verified codes where it has them (wdpm_dem_codes.hip); code, dem_grid*, dem_bounded describe it afterwards */
int encode_dem(wdpm_ctx *x);
/* `bytes` <= 32 bytes at the device address `src`, as of everything queued on the context's stream, are in `dst`: one copy through h_pin, one wait */
int read_back(wdpm_ctx *x, const void *src, void *dst, size_t bytes);

#endif
