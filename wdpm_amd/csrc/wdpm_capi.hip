/*
 * wdpm_capi.hip — the C ABI of include/wdpm.h implemented on HIP for gfx950: errors, the launch ledger, the context's life cycle,
 * every upload, download and peer copy, options.  The block loop is wdpm_block.hip, the DEM codes wdpm_dem_codes.hip, the
 * statistics wdpm_stats.hip; wdpm_ctx.h holds the context and what these units share.
 *
 * One context = one raster slab resident in one GPU's HBM for the context's lifetime:
 *   dem      rows x (C+2) fp64   read-only after upload; NODATA cells are rewritten to +inf on the device
 *   water[2] rows x (C+2) fp64   ping-pong pair (the fused kernel reads one, writes the other)
 *   old      rows x (C+2) fp64   snapshot for the convergence test
 *   scal     {totaldrain, olddrain} fp64 + one uint64 reduction cell
 * No CPU fallback: every compute entry point launches a HIP kernel or fails.
 */
#include <time.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <atomic>

#include "wdpm_ctx.h"

static thread_local char g_err[512] = "";

int wdpm_fail(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return 1;
}

/* Iter2Args::err: a wave of a two-iteration launch gave up waiting for another one - the rasters written since are wrong.  Sticky:
 * every later wait of this context fails too. */
static int wdpm_iter2_verdict(const wdpm_ctx *x) {
  if (x->h_iter2_err && *(volatile unsigned *)x->h_iter2_err)
    return wdpm_fail("a two-iteration launch (WDPM_ITER2) did not complete its hand-over between waves: results are invalid");
  return 0;
}

int wdpm_stream_sync(wdpm_ctx *x, hipStream_t s) {
  if (!x->comm) {
    const hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return wdpm_fail("hipStreamSynchronize failed: %s", hipGetErrorString(e));
    return wdpm_iter2_verdict(x);
  }
  static std::atomic<int> limit_ms{0};
  if (!limit_ms) { const char *t = getenv("WDPM_SYNC_TIMEOUT_S"); const double v = t ? atof(t) : 0.0; limit_ms = (int)((v > 0 ? v : 600.0) * 1000.0); }
  timespec t0;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  for (;;) {
    const hipError_t e = hipStreamQuery(s);
    if (e == hipSuccess) return wdpm_iter2_verdict(x);
    if (e != hipErrorNotReady) return wdpm_fail("hipStreamQuery failed: %s", hipGetErrorString(e));
    timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    const double ms = (double)(t.tv_sec - t0.tv_sec) * 1e3 + (double)(t.tv_nsec - t0.tv_nsec) * 1e-6;
    if (ms > (double)limit_ms) break;
    if (ms > 5.0) { const timespec nap{0, 100000}; nanosleep(&nap, nullptr); }   /* short waits spin, long ones nap 0.1 ms */
  }
  /* a halo transfer whose peer never sent (or died): end the communicator so that the queue drains, and say so */
  x->leak = true;
  (void)wdpm_comm_abort(x);
  return wdpm_fail("the GPU did not finish within %.0f s (WDPM_SYNC_TIMEOUT_S): a halo transfer did not complete; "
                   "the communicator was aborted", limit_ms / 1000.0);
}

/* The launch ledger (wdpm_ledger.h): filled in by the static initialisers of the kernel units when the library is loaded, counted
 * with relaxed atomics from then on.  Constant-initialised storage, so that registering from another unit's initialiser cannot
 * come before it exists. */
namespace {
constexpr int kLedgerMax = 128;
struct LedgerEntry {
  char name[96];
  std::atomic<long long> n[WDPM_LEDGER_SWITCH_STATES];
};
LedgerEntry g_ledger[kLedgerMax];
int g_ledger_entries = 0;       /* written by the loader's thread only, before any launch */
}  // namespace

int wdpm_ledger_register(const char *pretty, const char *args) {
  /* "const char *wdpm_ledger_pretty() [K = &(anonymous namespace)::fused_iteration_kernel]": the name after the last "::" */
  const char *k = strstr(pretty, "K = &");
  char name[96] = "?";
  if (k) {
    k += 5;
    size_t len = strcspn(k, ",]");
    for (const char *c = k; c < k + len; c++)
      if (c[0] == ':' && c[1] == ':') { len -= (size_t)(c + 2 - k); k = c + 2; c = k - 1; }
    snprintf(name, sizeof name, "%.*s%s", (int)len, k, args);
  }
  if (g_ledger_entries == kLedgerMax) return -1;       /* missing from the table: tests/test_launch_ledger.py says which */
  snprintf(g_ledger[g_ledger_entries].name, sizeof g_ledger[0].name, "%s", name);
  return g_ledger_entries++;
}

void wdpm_ledger_count(int slot, int switches) {
  if (slot >= 0) g_ledger[slot].n[switches & (WDPM_LEDGER_SWITCH_STATES - 1)].fetch_add(1, std::memory_order_relaxed);
}

/* The snapshot of a block is not a copy: wdpm_begin_block just declares the current raster to BE the
 * snapshot (old = cur) and owes it the threshold flush; the next iteration launch reads it - flushing
 * while it loads - and writes the other two rasters in turn, so the snapshot stays untouched until
 * wdpm_max_diff reads it (applying the same flush on the fly).  At 16384^2 that is 1.3 ms per block
 * that no longer exists.  Whoever needs the current raster flushed in memory, or wants to write
 * into it, asks for that first: */
int wdpm_tiles_touch(wdpm_ctx *x, int row, int nrows) {
  const int slot = x->cur;
  if (nrows > 0 && row < x->md_hi && row + nrows > x->md_lo) x->md_valid = false;   /* rows of the folded max diff */
  if (!x->zero_valid[slot] || nrows <= 0) return 0;
  if (x->tile_H < 6 || x->tile_nchunks < 1) { x->zero_valid[slot] = false; return 0; }
  /* chunk i's block is rows [H*i + 2 (0 for i = 0), H*(i+1) + 1] */
  int c0 = (row - 2) / x->tile_H, c1 = (row + nrows - 1 - 2) / x->tile_H;
  if (row < 2) c0 = 0;
  if (c0 < 0) c0 = 0;
  if (c1 > x->tile_nchunks - 1) c1 = x->tile_nchunks - 1;
  if (c1 < c0) return 0;
  const size_t pitch = (size_t)x->tile_nstrips + 2;
  HIP_TRY(hipMemset2DAsync(x->d_zero[slot] + (size_t)(c0 + 1) * pitch + 1, pitch, 0, (size_t)x->tile_nstrips, (size_t)(c1 - c0 + 1),
                           x->stream));
  return 0;
}

/* Drain module: drain() after each iteration (WDPMCL.c:1089) has no launch of its own either - the next
 * iteration launch applies it while loading (wdpm_march.hip, wdpm_small.hip: drain_owed).  Anybody else who looks at the
 * raster or at totaldrain gets it applied first.  (cur != old whenever it is owed: an iteration has run.) */
int wdpm_apply_owed_drain(wdpm_ctx *x) {
  if (!x->drain_owed) return 0;
  x->drain_owed = false;
  HIP_TRY(wdpm_launch_drain_outlet(x->d_w[x->cur], x->d_dem, x->g, x->d_scal, x->stream));
  return 0;
}

/* readers of d_w[cur]: the owed flush is applied in place (cur == old: the snapshot gets it too, idempotently) */
int wdpm_apply_owed_flush(wdpm_ctx *x) {
  if (wdpm_apply_owed_drain(x)) return 1;
  if (!x->flush_pending) return 0;
  HIP_TRY(wdpm_launch_flush_snapshot(x->d_w[x->cur], x->d_w[x->cur], x->cells, x->flush_thres, x->stream));
  x->flush_pending = false;
  flushed_whole(x, x->flush_thres);
  return 0;
}

/* in-place writers of d_w[cur] (pass kernels, drain(), partial uploads): the snapshot must survive */
int ensure_private(wdpm_ctx *x) {
  x->md_valid = false;             /* whoever asks is about to write into the raster */
  if (wdpm_apply_owed_drain(x)) return 1;
  if (x->cur != x->old) return 0;
  const int t = free_slot(x);
  if (x->flush_pending) {
    HIP_TRY(wdpm_launch_flush_snapshot(x->d_w[x->cur], x->d_w[t], x->cells, x->flush_thres, x->stream));
    x->flush_pending = false;
    flushed_whole(x, x->flush_thres);      /* (the copy that becomes current is the flushed one) */
  } else {
    HIP_TRY(hipMemcpyAsync(x->d_w[t], x->d_w[x->cur], x->cells * sizeof(double), hipMemcpyDeviceToDevice, x->stream));
  }
  x->zero_valid[t] = false;      /* a copy: its flags could be copied too, but whoever asked is about to write into it */
  x->cur = t;
  return 0;
}

/* a whole new raster is about to be written: no copy needed, just do not overwrite the snapshot */
int ensure_fresh_slot(wdpm_ctx *x) {
  if (wdpm_apply_owed_flush(x)) return 1;
  if (x->cur == x->old) x->cur = free_slot(x);
  x->zero_valid[x->cur] = false;
  x->md_valid = false;
  return 0;
}

int read_back(wdpm_ctx *x, const void *src, void *dst, size_t bytes) {
  if (bytes > 4 * sizeof(double)) return wdpm_fail("read_back: %zu bytes do not fit the pinned staging words", bytes);
  HIP_TRY(hipMemcpyAsync(x->h_pin, src, bytes, hipMemcpyDeviceToHost, x->stream));
  if (wdpm_stream_sync(x, x->stream)) return 1;
  memcpy(dst, x->h_pin, bytes);
  return 0;
}

/* Guard bands (debugging aid, WDPM_GUARD_KB=<n> in the environment when the context is made): the big device buffers - DEM,
 * the three water rasters, the DEM codes, the tile flags - get n KiB of 0xA5 bytes in front and behind, and
 * wdpm_get_option(WDPM_OPT_GUARD_BAD) counts guard bytes that no longer hold 0xA5: a kernel writing outside its raster shows up
 * there even when the stray bytes land in nobody's data.  The GPU pool has no address sanitizer; the fuzz tests run with this on. */
static size_t guard_bytes() {
  static std::atomic<long> kb{-1};
  if (kb < 0) { const char *e = getenv("WDPM_GUARD_KB"); kb = e ? atol(e) : 0; if (kb < 0) kb = 0; }
  return (size_t)kb * 1024;
}
static hipError_t guarded_malloc(wdpm_ctx *x, void **p, size_t bytes) {
  const size_t g = guard_bytes();
  char *base = nullptr;
  hipError_t e = hipMalloc(&base, bytes + 2 * g);
  if (e != hipSuccess) return e;
  if (g) {
    e = hipMemset(base, 0xA5, g);
    if (e == hipSuccess) e = hipMemset(base + g + bytes, 0xA5, g);
    if (e != hipSuccess) { (void)hipFree(base); return e; }
    x->guards.push_back({base, bytes});
  }
  *p = base + g;
  return hipSuccess;
}
static void guarded_free(void *p) {
  if (p) (void)hipFree(static_cast<char *>(p) - guard_bytes());
}
static int guard_damage(wdpm_ctx *x, int64_t *bad) {
  *bad = 0;
  const size_t g = guard_bytes();
  if (!g || x->guards.empty()) return 0;
  if (bind(x)) return 1;
  if (wdpm_stream_sync(x, x->stream)) return 1;
  if (x->side && wdpm_stream_sync(x, x->side)) return 1;
  std::vector<unsigned char> h(g);
  for (const auto &gb : x->guards)
    for (int side = 0; side < 2; side++) {
      HIP_TRY(hipMemcpy(h.data(), gb.base + (side ? g + gb.bytes : 0), g, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < g; i++) *bad += h[i] != 0xA5;
    }
  return 0;
}

/* after water has been written to rows [row, row+nrows): the kinds of depth it holds (wdpm_launch_scan_water) join what is known */
static int note_water_kinds(wdpm_ctx *x, int row, int nrows) {
  const size_t off = (size_t)row * x->g.ncp;
  HIP_TRY(hipMemsetAsync(x->d_bits, 0, sizeof(unsigned long long), x->stream));
  HIP_TRY(wdpm_launch_scan_water(x->d_w[x->cur] + off, x->d_dem + off, (size_t)nrows * x->g.ncp, x->d_bits, x->stream));
  unsigned long long found;
  if (read_back(x, x->d_bits, &found, sizeof found)) return 1;
  x->kinds |= (unsigned)found & (WDPM_WATER_NEGZERO | WDPM_WATER_NEGATIVE | WDPM_WATER_ODD);
  return 0;
}

/* Direct peer access between two devices, asked for once per ordered pair: without it
 * hipMemcpyPeerAsync silently stages through host memory on ROCm.  A refusal (no xGMI/PCIe path) is
 * remembered and leaves the staged copy in charge - slower, same bits. */
static int enable_peer(int dev, int peer) {
  static signed char state[64][64];   /* 0 unknown, 1 enabled, -1 refused */
  if (dev == peer || dev < 0 || peer < 0 || dev >= 64 || peer >= 64 || state[dev][peer]) return 0;
  int can = 0;
  HIP_TRY(hipSetDevice(dev));
  HIP_TRY(hipDeviceCanAccessPeer(&can, dev, peer));
  if (can) {
    const hipError_t e = hipDeviceEnablePeerAccess(peer, 0);
    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) can = 0;
    (void)hipGetLastError();
  }
  state[dev][peer] = can ? 1 : -1;
  if (!can) fprintf(stderr, "wdpm: no direct peer access from device %d to device %d; halo copies are staged\n", dev, peer);
  return 0;
}

extern "C" {

int wdpm_launch_ledger(int32_t index, const char **name, int64_t *launches, int64_t *by_switches) {
  if (index < 0 || index >= g_ledger_entries) return g_ledger_entries;
  long long total = 0;
  for (int i = 0; i < WDPM_LEDGER_SWITCH_STATES; i++) {
    const long long v = g_ledger[index].n[i].load(std::memory_order_relaxed);
    total += v;
    if (by_switches) by_switches[i] = v;
  }
  if (name) *name = g_ledger[index].name;
  if (launches) *launches = total;
  return g_ledger_entries;
}

const char *wdpm_last_error(void) { return g_err; }
void wdpm_set_last_error(const char *msg) { snprintf(g_err, sizeof g_err, "%s", msg ? msg : ""); }
const char *wdpm_backend_name(void) { return "hip-gfx950"; }
int wdpm_abi_version(void) { return WDPM_ABI_VERSION; }

int wdpm_create(wdpm_ctx **out, const wdpm_params *p) {
  if (!out || !p) return wdpm_fail("wdpm_create: null argument");
  if (p->nrows < 1 || p->ncols < 1) return wdpm_fail("wdpm_create: bad raster size %d x %d", p->nrows, p->ncols);
  if (p->module < WDPM_ADD || p->module > WDPM_DRAIN) return wdpm_fail("wdpm_create: bad module %d", p->module);
  if (p->kernel < WDPM_KERNEL_AUTO || p->kernel > WDPM_KERNEL_FUSED) return wdpm_fail("wdpm_create: bad kernel selector %d", p->kernel);
  if (p->slab_row0 < 0 || p->slab_row0 % 3 != 0) return wdpm_fail("wdpm_create: slab_row0 must be a non-negative multiple of 3");
  const int rows = p->slab_rows > 0 ? p->slab_rows : p->nrows + 2;
  if (p->slab_row0 + rows > p->nrows + 2) return wdpm_fail("wdpm_create: slab exceeds raster");
  if (rows < 3) return wdpm_fail("wdpm_create: a slab needs at least 3 rows");
  if ((double)rows * (double)(p->ncols + 2) > 2.0e9) return wdpm_fail("wdpm_create: raster too large: a row block takes at most 2e9 cells (%d rows x %d here; use more row blocks)", rows, p->ncols + 2);
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (ndev < 1) return wdpm_fail("wdpm_create: no HIP device (this library has no CPU fallback)");
  if (p->device < 0 || p->device >= ndev) return wdpm_fail("wdpm_create: device %d out of range (%d devices)", p->device, ndev);
  HIP_TRY(hipSetDevice(p->device));
  const DeviceFacts *facts = wdpm_device_facts();       /* of p->device: queried when its first context is created */
  if (!facts) return wdpm_fail("wdpm_create: device %d: no facts for the launch planner", p->device);

  wdpm_ctx *x = new wdpm_ctx();       /* every member at its default (wdpm_ctx.h) */
  x->p = *p;
  x->facts = facts;
  x->g.rows = rows;
  x->g.ncp = p->ncols + 2;
  x->g.row0 = p->slab_row0;
  x->g.R = p->nrows;
  x->g.C = p->ncols;
  x->g.dr = p->drainrow - p->slab_row0;
  x->g.dc = p->draincol;
  x->g.miss = p->missingvalue;
  if (p->module != WDPM_DRAIN) { x->g.dr = -1000000; x->g.dc = -1000000; }
  x->cells = (size_t)rows * x->g.ncp;
  x->kernel = p->kernel;
  if (x->kernel == WDPM_KERNEL_AUTO) {
    /* The one-iteration kernel; WDPM_KERNEL=pass|fused selects one explicitly.  (Round 1 also carried two
     * two-iterations-per-launch kernels: -0.5 % .. +8 % against this one depending on slab shape and box,
     * VALU-bound; they were taken out of the product in round 2 - DESIGN.md §7b.) */
    x->kernel = WDPM_KERNEL_FUSED;
    if (const char *e = getenv("WDPM_KERNEL")) {
      if (!strcmp(e, "pass")) x->kernel = WDPM_KERNEL_PASS;
      else if (!strcmp(e, "fused")) x->kernel = WDPM_KERNEL_FUSED;
    }
  }
  if (const char *e = getenv("WDPM_TILES")) x->tiles_mode = atoi(e);
  const size_t bytes = x->cells * sizeof(double);
  hipError_t e = hipStreamCreateWithFlags(&x->stream, hipStreamNonBlocking);
  /* the side stream carries the interior launch of wdpm_iterate_overlapped: lowest priority, so that
   * the boundary launches on the main stream (whose rows a neighbour is waiting for) get the CUs first */
  int prio_least = 0, prio_greatest = 0;
  if (e == hipSuccess) e = hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
  if (e == hipSuccess) e = hipStreamCreateWithPriority(&x->side, hipStreamNonBlocking, prio_least);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&x->ev_fork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&x->ev_join, hipEventDisableTiming);
  if (e == hipSuccess) e = guarded_malloc(x, (void **)&x->d_dem, bytes + kRasterSpare);
  for (int i = 0; i < 3 && e == hipSuccess; i++) e = guarded_malloc(x, (void **)&x->d_w[i], bytes + kRasterSpare);
  if (e == hipSuccess) e = guarded_malloc(x, (void **)&x->d_dem32, x->cells * sizeof(int) + 64);
  if (e == hipSuccess) e = guarded_malloc(x, (void **)&x->d_dem16, x->cells * sizeof(unsigned short) + 64);
  if (e == hipSuccess) e = guarded_malloc(x, (void **)&x->d_gbase, (size_t)x->g.rows * dem_groups(x->g.ncp) * sizeof(int) + 64);
  if (e == hipSuccess) e = hipMalloc(&x->d_scal, 2 * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&x->d_bits, 3 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMalloc(&x->d_md, sizeof(unsigned long long));
  if (e == hipSuccess) {
    /* chunk heights by what each XCD delivers (wdpm_kernels.h::XcdBalance).  WDPM_BALANCE=0: equal heights always; 2: the table on
     * launches of any size, starting from deliberately skewed weights (the parity suites under it) */
    const char *be = getenv("WDPM_BALANCE");
    x->bal.mode = be ? atoi(be) : 1;
    if (x->bal.mode < 0 || x->bal.mode > 2) x->bal.mode = 1;
    x->bal.capacity = 16384;
    if (x->bal.mode) {
      static const float even[kBalClasses] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 0.95f, 1.f};
      static const float skew[kBalClasses] = {0.8f, 1.2f, 0.9f, 1.1f, 1.25f, 0.75f, 1.0f, 1.0f, 0.8f, 1.15f};
      e = hipMalloc(&x->bal.table, (size_t)x->bal.capacity * sizeof(int));
      if (e == hipSuccess) e = hipMalloc(&x->bal.acc, (2 * kBalClasses + 2) * sizeof(unsigned long long));
      if (e == hipSuccess) e = hipMalloc(&x->bal.weight, kBalClasses * sizeof(float));
      if (e == hipSuccess) e = hipMemsetAsync(x->bal.acc, 0, (2 * kBalClasses + 2) * sizeof(unsigned long long), x->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(x->bal.weight, x->bal.mode == 2 ? skew : even, kBalClasses * sizeof(float), hipMemcpyHostToDevice, x->stream);
    }
  }
  {
    /* tile flags: strips of 171 columns x chunks of >= 6 rows */
    x->tile_cap = (x->g.ncp / 171 + 4) * (rows / 6 + 4);
    for (int i = 0; i < 3 && e == hipSuccess; i++) e = guarded_malloc(x, (void **)&x->d_zero[i], (size_t)x->tile_cap);
    if (e == hipSuccess) e = hipMalloc(&x->d_active, sizeof(unsigned));
    if (e == hipSuccess) e = hipHostMalloc(&x->h_active, sizeof(unsigned));
    if (e == hipSuccess) e = hipMemsetAsync(x->d_active, 0, sizeof(unsigned), x->stream);
  }
  if (e == hipSuccess) e = hipHostMalloc(&x->h_pin, 4 * sizeof(double));
  if (e == hipSuccess) e = hipHostMalloc(&x->h_iter2_err, sizeof(unsigned), hipHostMallocMapped);
  if (e == hipSuccess) { *x->h_iter2_err = 0u; e = hipHostGetDevicePointer((void **)&x->d_iter2_err, x->h_iter2_err, 0); }
  if (e == hipSuccess) e = hipMemsetAsync(x->d_scal, 0, 2 * sizeof(double), x->stream);
  if (e == hipSuccess) e = hipMemsetAsync(x->d_w[2], 0, bytes, x->stream);   /* the snapshot before any block: zeros */
  if (e == hipSuccess) e = hipStreamSynchronize(x->stream);
  if (e != hipSuccess) {
    wdpm_fail("wdpm_create: device allocation failed: %s", hipGetErrorString(e));
    wdpm_destroy(x);
    return 1;
  }
  *out = x;
  return 0;
}

void wdpm_destroy(wdpm_ctx *x) {
  if (!x) return;
  (void)hipSetDevice(x->p.device);
  if (!x->leak) (void)wdpm_stream_sync(x, x->stream);
  wdpm_comm_release(x);
  if (x->leak) return;           /* a stuck transfer or helper thread may still touch the stream and the buffers: nothing is freed */
  if (x->side) { (void)hipStreamSynchronize(x->side); (void)hipStreamDestroy(x->side); }
  if (x->ev_fork) (void)hipEventDestroy(x->ev_fork);
  if (x->ev_join) (void)hipEventDestroy(x->ev_join);
  for (int i = 0; i < 2; i++)
    if (x->ev_copy[i]) (void)hipEventDestroy(x->ev_copy[i]);
  for (auto &ge : x->graphs) (void)hipGraphExecDestroy(ge.exec);
  for (auto *t : x->timers()) x->pool.insert(x->pool.end(), t->pending.begin(), t->pending.end());   /* recorded, never read */
  for (auto &ep : x->pool) { (void)hipEventDestroy(ep.a); (void)hipEventDestroy(ep.b); }
  guarded_free(x->d_dem); guarded_free(x->d_w[0]); guarded_free(x->d_w[1]); guarded_free(x->d_w[2]);
  (void)hipFree(x->d_scal); (void)hipFree(x->d_bits); guarded_free(x->d_dem32); (void)hipFree(x->d_stat);
  guarded_free(x->d_dem16); guarded_free(x->d_gbase);
  for (int i = 0; i < 3; i++) guarded_free(x->d_zero[i]);
  (void)hipFree(x->d_active);
  (void)hipFree(x->d_md);
  (void)hipFree(x->bal.table); (void)hipFree(x->bal.acc); (void)hipFree(x->bal.weight);
  if (x->h_active) (void)hipHostFree(x->h_active);
  if (x->h_pin) (void)hipHostFree(x->h_pin);
  if (x->h_iter2_err) (void)hipHostFree(x->h_iter2_err);
  (void)hipFree(x->d_sum_approx); (void)hipFree(x->d_sum_i); (void)hipFree(x->d_sum_k); (void)hipFree(x->d_sum_flag);
  if (x->own_stream && x->stream) (void)hipStreamDestroy(x->stream);
  delete x;
}

int wdpm_set_stream(wdpm_ctx *x, void *hip_stream) {
  if (bind(x)) return 1;   /* also joins a pending interior launch onto the old stream */
  if (wdpm_stream_sync(x, x->stream)) return 1;
  if (x->own_stream && x->stream) HIP_TRY(hipStreamDestroy(x->stream));
  x->stream = (hipStream_t)hip_stream;
  x->own_stream = false;
  return 0;
}

int wdpm_synchronize(wdpm_ctx *x) {
  if (bind(x)) return 1;
  if (wdpm_stream_sync(x, x->stream)) return 1;
  return 0;
}

/* ---- data movement ---------------------------------------------------------------------- */
int wdpm_upload(wdpm_ctx *x, const double *bigdem, const double *bigwater) {
  if (!bigdem || !bigwater) return wdpm_fail("wdpm_upload: null array");
  if (bind(x)) return 1;
  const size_t bytes = x->cells * sizeof(double);
  if (ensure_fresh_slot(x)) return 1;
  HIP_TRY(hipMemcpyAsync(x->d_dem, bigdem, bytes, hipMemcpyHostToDevice, x->stream));
  HIP_TRY(hipMemcpyAsync(x->d_w[x->cur], bigwater, bytes, hipMemcpyHostToDevice, x->stream));
  HIP_TRY(wdpm_launch_mark_nodata(x->d_dem, x->cells, x->g.miss, x->stream));
  x->kinds = 0;                            /* a whole new raster: what the scan finds, nothing else */
  if (note_water_kinds(x, 0, x->g.rows)) return 1;
  if (encode_dem(x)) return 1;
  return 0;
}

/* Set-up on the device: the slab's padded rasters straight from the UNPADDED file rasters.
 * The two water rasters that are not current serve as staging for the host-to-device copies. */
int wdpm_upload_unpadded(wdpm_ctx *x, const double *dem, const double *water, const wdpm_setup *su) {
  if (!dem || !su) return wdpm_fail("wdpm_upload_unpadded: null argument");
  if (su->op < 0 || su->op > 2) return wdpm_fail("wdpm_upload_unpadded: bad water operation %d", su->op);
  if (bind(x)) return 1;
  if (ensure_fresh_slot(x)) return 1;
  const int a = (x->cur + 1) % 3, b = (x->cur + 2) % 3;
  x->zero_valid[a] = x->zero_valid[b] = false;
  const int R = x->g.R, C = x->g.C;
  int f0 = x->g.row0 - 1, f1 = x->g.row0 + x->g.rows - 2;     /* file rows behind the slab's padded rows */
  const int first = f0 < 0 ? 0 : f0, last = f1 > R - 1 ? R - 1 : f1;
  if (last >= first) {
    const size_t off = (size_t)(first - f0) * C, n = (size_t)(last - first + 1) * C;
    HIP_TRY(hipMemcpyAsync(x->d_w[a] + off, dem + (size_t)first * C, n * sizeof(double), hipMemcpyHostToDevice, x->stream));
    if (water)
      HIP_TRY(hipMemcpyAsync(x->d_w[b] + off, water + (size_t)first * C, n * sizeof(double), hipMemcpyHostToDevice, x->stream));
  }
  HIP_TRY(wdpm_launch_pad_setup(x->d_w[a], water ? x->d_w[b] : nullptr, x->d_dem, x->d_w[x->cur], x->g, su->op, su->add,
                                su->rof, su->sub, x->stream));
  /* the snapshot before any block is all zeros (as after wdpm_create) */
  x->old = a;
  x->flush_thres = -__builtin_inf();
  HIP_TRY(hipMemsetAsync(x->d_w[a], 0, x->cells * sizeof(double), x->stream));
  x->kinds = 0;
  if (note_water_kinds(x, 0, x->g.rows)) return 1;
  return encode_dem(x);
}

int wdpm_set_drain(wdpm_ctx *x, int32_t drainrow, int32_t draincol) {
  if (x->p.module != WDPM_DRAIN) return wdpm_fail("wdpm_set_drain: not a drain context");
  if (bind(x) || wdpm_apply_owed_drain(x)) return 1;
  x->p.drainrow = drainrow;
  x->p.draincol = draincol;
  x->g.dr = drainrow - x->p.slab_row0;
  x->g.dc = draincol;
  return 0;
}

int wdpm_download_unpadded(wdpm_ctx *x, int32_t file_row, int32_t nrows, int32_t mask_missing, double *dst) {
  const int p0 = file_row + 1 - x->g.row0;                      /* slab-local padded row of the first file row */
  if (nrows < 0 || file_row < 0 || file_row + nrows > x->g.R || p0 < 0 || p0 + nrows > x->g.rows || !dst)
    return wdpm_fail("wdpm_download_unpadded: rows outside the slab");
  if (nrows == 0) return 0;
  if (bind(x) || wdpm_apply_owed_flush(x)) return 1;
  const int st = free_slot(x);
  double *stage = x->d_w[st];
  x->zero_valid[st] = false;
  HIP_TRY(wdpm_launch_unpad(x->d_w[x->cur], x->d_dem, x->g, file_row, nrows, mask_missing, stage, x->stream));
  HIP_TRY(hipMemcpyAsync(dst, stage, (size_t)nrows * x->g.C * sizeof(double), hipMemcpyDeviceToHost, x->stream));
  if (wdpm_stream_sync(x, x->stream)) return 1;
  return 0;
}

int wdpm_upload_water(wdpm_ctx *x, const double *bigwater) {
  if (!bigwater) return wdpm_fail("wdpm_upload_water: null array");
  if (bind(x)) return 1;
  if (ensure_fresh_slot(x)) return 1;
  HIP_TRY(hipMemcpyAsync(x->d_w[x->cur], bigwater, x->cells * sizeof(double), hipMemcpyHostToDevice, x->stream));
  x->kinds = 0;
  return note_water_kinds(x, 0, x->g.rows);
}

int wdpm_download_water(wdpm_ctx *x, double *bigwater) {
  if (!bigwater) return wdpm_fail("wdpm_download_water: null array");
  if (bind(x)) return 1;
  if (wdpm_apply_owed_flush(x)) return 1;
  HIP_TRY(hipMemcpyAsync(bigwater, x->d_w[x->cur], x->cells * sizeof(double), hipMemcpyDeviceToHost, x->stream));
  if (wdpm_stream_sync(x, x->stream)) return 1;
  return 0;
}

int wdpm_download_rows(wdpm_ctx *x, int32_t row, int32_t nrows, double *dst) {
  if (!rows_inside(x, row, row + nrows) || !dst) return wdpm_fail("wdpm_download_rows: bad row range");
  if (bind(x)) return 1;
  if (wdpm_apply_owed_flush(x)) return 1;
  HIP_TRY(hipMemcpyAsync(dst, x->d_w[x->cur] + (size_t)row * x->g.ncp, (size_t)nrows * x->g.ncp * sizeof(double),
                         hipMemcpyDeviceToHost, x->stream));
  if (wdpm_stream_sync(x, x->stream)) return 1;
  return 0;
}

int wdpm_upload_rows(wdpm_ctx *x, int32_t row, int32_t nrows, const double *src) {
  if (!rows_inside(x, row, row + nrows) || !src) return wdpm_fail("wdpm_upload_rows: bad row range");
  if (bind(x)) return 1;
  if (ensure_private(x)) return 1;
  x->zero_valid[x->cur] = false;
  HIP_TRY(hipMemcpyAsync(x->d_w[x->cur] + (size_t)row * x->g.ncp, src, (size_t)nrows * x->g.ncp * sizeof(double),
                         hipMemcpyHostToDevice, x->stream));
  return note_water_kinds(x, row, nrows);   /* only adds: the other rows hold what they held */
}

int wdpm_enable_peer_access(wdpm_ctx *a, wdpm_ctx *b) {
  if (!a || !b) return wdpm_fail("wdpm_enable_peer_access: null context");
  if (enable_peer(a->p.device, b->p.device)) return 1;
  return enable_peer(b->p.device, a->p.device);
}

int wdpm_copy_rows(wdpm_ctx *dst, int32_t dst_row, wdpm_ctx *src, int32_t src_row, int32_t nrows) {
  if (!dst || !src || dst->g.ncp != src->g.ncp || !rows_inside(dst, dst_row, dst_row + nrows) || !rows_inside(src, src_row, src_row + nrows))
    return wdpm_fail("wdpm_copy_rows: bad row range");
  if (nrows == 0) return 0;
  if (src->p.device != dst->p.device && wdpm_enable_peer_access(dst, src)) return 1;
  /* Ordered on the device, never on the host: the copy runs on the destination's stream behind
   * everything queued there (its kernels are done with the rows being overwritten), after an event
   * that marks the source's queue (its kernels have produced the rows); the source's later work in
   * turn waits for the copy to have read them.  With N devices in a chain the halo refresh is then
   * 2(N-1) enqueues and no host round trip. */
  if (bind(src)) return 1;                       /* also joins a pending overlapped interior launch */
  /* Rows that leave a context carry the last iteration's drain(): the receiver applies its own owed drain() only where the
   * outlet lies strictly inside ITS slab - not when the outlet's row is the slab's first or last row, and then the nine
   * cells must arrive zeroed (tests/test_rowblock.py::test_hip_outlet_on_the_last_row_of_the_neighbours_halo). */
  if (wdpm_apply_owed_flush(src)) return 1;   /* ... and the block's threshold flush, should the source still owe it to its raster */
  /* ... and what kinds of depth the source may hold travel with the rows: a caller who peer-copies rows with a -0.0, a
   * negative or an odd depth into a context whose own scan was clean must not leave it on the gate-free kernel variants */
  dst->kinds |= src->kinds;
  if (!src->ev_copy[0]) HIP_TRY(hipEventCreateWithFlags(&src->ev_copy[0], hipEventDisableTiming));
  HIP_TRY(hipEventRecord(src->ev_copy[0], src->stream));
  if (bind(dst)) return 1;
  if (!dst->ev_copy[1]) HIP_TRY(hipEventCreateWithFlags(&dst->ev_copy[1], hipEventDisableTiming));
  HIP_TRY(hipStreamWaitEvent(dst->stream, src->ev_copy[0], 0));
  if (wdpm_tiles_touch(dst, dst_row, nrows)) return 1;       /* queued on dst's stream, ahead of the copy */
  EventPair xep;
  if (wdpm_xch_timing_begin(dst, &xep)) return 1;
  const size_t bytes = (size_t)nrows * src->g.ncp * sizeof(double);
  double *d = dst->d_w[dst->cur] + (size_t)dst_row * dst->g.ncp;
  const double *s = src->d_w[src->cur] + (size_t)src_row * src->g.ncp;
  if (src->p.device == dst->p.device) HIP_TRY(hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToDevice, dst->stream));
  else HIP_TRY(hipMemcpyPeerAsync(d, dst->p.device, s, src->p.device, bytes, dst->stream));
  if (wdpm_xch_timing_end(dst, &xep)) return 1;
  HIP_TRY(hipEventRecord(dst->ev_copy[1], dst->stream));
  HIP_TRY(hipSetDevice(src->p.device));
  HIP_TRY(hipStreamWaitEvent(src->stream, dst->ev_copy[1], 0));
  return 0;
}

int wdpm_get_option(wdpm_ctx *x, int32_t key, int64_t *value) {
  if (!value) return wdpm_fail("wdpm_get_option: null argument");
  if (key == WDPM_OPT_SIGNED_ZERO_SAFE) *value = x->negzero() ? 1 : 0;
  else if (key == WDPM_OPT_WATER_KINDS) *value = x->kinds;
  else if (key == WDPM_OPT_PLAIN_WATER) *value = wdpm_switches().plain != 0 && x->plain() ? 1 : 0;
  else if (key == WDPM_OPT_DEM32) *value = x->code.q ? 1 : 0;
  else if (key == WDPM_OPT_DEM16) *value = x->code.q && x->code.h ? (wdpm_dem16_pays((long long)x->cells, x->code.force) ? 1 : 2) : 0;   /* 2: available, but a whole-slab launch of this size keeps the 32-bit codes */
  else if (key == WDPM_OPT_TILES) *value = x->tiles_mode;
  else if (key == WDPM_OPT_TILES_SEEN) *value = x->stat_tiles;
  else if (key == WDPM_OPT_TILES_WORKED) *value = x->stat_active;
  else if (key == WDPM_OPT_SPARSE) *value = x->sparse ? 1 : 0;
  else if (key == WDPM_OPT_GRAPH_LAUNCHES) *value = x->graph_launches;
  else if (key == WDPM_OPT_DEM_GRID) *value = x->dem_grid;          /* what upload found, whatever WDPM_OPT_DEM32 was set to since */
  else if (key == WDPM_OPT_DEM_GRID_EXP) *value = x->dem_grid_exp;
  else if (key == WDPM_OPT_GUARD_BAD) return guard_damage(x, value);
  else return wdpm_fail("wdpm_get_option: unknown option %d", key);
  return 0;
}

int wdpm_set_option(wdpm_ctx *x, int32_t key, int64_t value) {
  drop_graphs(x);
  if (key == WDPM_OPT_SIGNED_ZERO_SAFE) {
    x->kinds = value != 0 ? x->kinds | WDPM_WATER_NEGZERO : x->kinds & ~(unsigned)WDPM_WATER_NEGZERO;
  } else if (key == WDPM_OPT_WATER_KINDS) {        /* OR-ed in: what a multi-GPU driver found on the other ranks */
    x->kinds |= (unsigned)value & (WDPM_WATER_NEGZERO | WDPM_WATER_NEGATIVE | WDPM_WATER_ODD);
  } else if (key == WDPM_OPT_DEM32 || key == WDPM_OPT_DEM16) {
    /* switching the codes on is honoured only for a DEM that passed the device's bit-for-bit check; the 16-bit offsets are
     * offsets of the 32-bit codes, so they follow them, and offsets, group bases and their pitch go on and off together */
    if (key == WDPM_OPT_DEM32) {
      x->code.q = (value != 0 && x->dem32_encodable) ? x->d_dem32 : nullptr;
      x->code.force = value == 2;   /* 2: also on launches too small for the codes to pay (tests) */
    } else {
      x->dem16_wanted = value != 0;
    }
    const bool on16 = x->dem16_wanted && x->dem16_encodable && x->code.q != nullptr;
    x->code.h = on16 ? x->d_dem16 : nullptr;
    x->code.gb = on16 ? x->d_gbase : nullptr;
    x->code.ngroups = on16 ? dem_groups(x->g.ncp) : 0;
  } else if (key == WDPM_OPT_TILES) {
    x->tiles_mode = value != 0;
    x->zero_valid[0] = x->zero_valid[1] = x->zero_valid[2] = false;
  } else if (key == WDPM_OPT_SPARSE) {
    x->sparse = value != 0;
  } else {
    return wdpm_fail("wdpm_set_option: unknown option %d", key);
  }
  return 0;
}

int wdpm_water_ptr(wdpm_ctx *x, void **ptr) {
  if (bind(x) || ensure_private(x)) return 1;   /* the caller may write through it */
  x->zero_valid[x->cur] = false;
  x->kinds |= WDPM_WATER_ODD;                    /* ... anything at all: the gated kernel variants from here on */
  *ptr = x->d_w[x->cur];
  return 0;
}
int wdpm_dem_ptr(wdpm_ctx *x, void **ptr) {
  x->dem_bounded = false;                        /* the caller may write anything through it */
  *ptr = x->d_dem;
  return 0;
}

int wdpm_host_alloc(size_t bytes, void **ptr) {
  if (!ptr) return wdpm_fail("wdpm_host_alloc: null argument");
  *ptr = nullptr;
  HIP_TRY(hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocPortable));
  return 0;
}

void wdpm_host_free(void *ptr) {
  if (ptr) (void)hipHostFree(ptr);
}

int wdpm_device_info(wdpm_ctx *x, int32_t *ordinal, char *pci_bus_id, int32_t len) {
  if (ordinal) *ordinal = x->p.device;
  if (pci_bus_id) {
    if (len < 16) return wdpm_fail("wdpm_device_info: the PCI bus id needs 16 bytes, got %d", (int)len);
    HIP_TRY(hipDeviceGetPCIBusId(pci_bus_id, len, x->p.device));
  }
  return 0;
}

} /* extern "C" */
