/*
 * wdpm_pond_curves.hip — the stage curve of every pond (include/wdpm_pond_curves.h): the lowest ground of the pond's basin, and the
 * cells and the storage of the basin below sixteen levels between that bed and the pond's pour level; from the basin raster, the DEM
 * and the outlet table a wdpm_outlets_label leaves on the device.  gfx950.  A unit of its own beside wdpm_ponds.hip,
 * wdpm_pond_rims.hip, wdpm_pond_catchments.hip and wdpm_pond_outlets.hip: not in the launch ledger, not among the sources
 * wdpm_build_info() hashes.
 *
 * A wave owns one 64-column segment over rows_per_wave rows (ponds_rows_per_wave), as in the other units.  Neither pass has a
 * stencil - a cell wants its own basin and its own dem - so there is no window and no exchange of columns.
 *
 *   init     bed keys to the maximum, the pour level of the outlet table into top_level, counts and sums to zero
 *   bed      a row's basins; a row with no basin > 0 reads no dem.  Otherwise per wave BY LABEL a butterfly minimum of the dem keys,
 *            carried down the rows while the label stays, and one atomic_min_if on the pond's bed key per (wave, label change)
 *   stages   after every bed key is final.  A lane keeps bed and top of its own basin and reloads them only when its basin differs
 *            from the one it held; a row whose lanes hold no basin > 0 with a finite top reads the basins alone, and one whose
 *            cells all stand at or above their top is done after its dem.  The sixteen heights are formed by the rule of
 *            wdpm_curves_stage_level, and every lane adds its cell to sixteen counts and sixteen sums of its own, all in
 *            registers (the stage loops are unrolled: nothing is indexed at run time).  What the lanes hold for one label goes
 *            out when a lane's label changes, and at the end of the strip: per wave BY LABEL a butterfly sum per stage and one add
 *            of the count and one of the sum to the pond's row; a stage whose count is zero in the wave sends nothing.  Counts
 *            and sums are cumulative as they are defined, there is no prefix sum afterwards.  A term of 512 m or more, or one
 *            that is not finite, sets a status word
 *   finish   the bed key back to a double; the counts for wdpm_curves_stats
 *
 * Over row blocks (include/wdpm_group_pond_curves.h) every rank runs the same bodies over its owned rows (kRows) and never reads a row
 * beyond them.  The table is indexed through the label -> slot table of the rims and catchments: once per (wave, label change) in the
 * bed pass, at the per-lane reload and at the send in the stage pass.  The bed key must be final over ALL ranks before a stage height
 * is formed, so the host stands between bed and stages (wdpm_curves_merge.h): the ranks' keys come down, the lowest per pond goes back
 * up - still a key; the host alone turns it into a double, once per pond - and there is no finish on the device.  The top level is
 * the pour key the group's outlet pass left in every slot's outlet row.
 *
 * Everything that steers a loop is wave-uniform.  tests/curves_emu_main.cpp and tests/group_curves_emu_main.cpp compile the kernels for
 * the host under sanitizers with WDPM_PONDS_EMULATION defined, as tests/outlets_emu_main.cpp does with wdpm_pond_outlets.hip, and leave
 * the host half out.
 */
#include "wdpm_ponds_priv.h"

using namespace wdpm_pond_detail;

#ifdef __clang__
#pragma clang fp contract(off)            /* the stage rule is three rounded operations, whatever the command line says */
#endif
#ifdef WDPM_PONDS_EMULATION
#define WDPM_CURVES_BOTH
#else
#define WDPM_CURVES_BOTH __host__ __device__
#endif

namespace {

constexpr unsigned long long kNoBed = ~0ull;      /* no cell of the basin seen yet */
constexpr int kStages = WDPM_CURVE_STAGES;

/* The stage rule of include/wdpm_pond_curves.h for 0 < s < 16: one subtraction, one multiplication by the exact s / 16, one
 * addition.  Device, host and the host emulation all come here. */
WDPM_CURVES_BOTH inline double stage_between(double bed, double top, int s) {
  const double span = top - bed;
  const double part = span * ((double)s * 0.0625);
  return bed + part;
}

/* butterflies: every lane ends with the wave's sum */
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

/* ---- init ------------------------------------------------------------------------------------------------------------------ */
/* one thread per 64-bit word of the table: word 0 of a row is the bed key, word 1 the top level, the rest counts and sums */
__global__ __launch_bounds__(kBlock) void curves_init_kernel(CurveRow *t, long long n, const wdpm_pond_outlet *__restrict__ outlets) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n * kCurveWords) return;
  const long long k = i / kCurveWords;
  const int j = (int)(i - k * kCurveWords);
  unsigned long long v = 0ull;
  if (j == 0) v = kNoBed;
  if (j == 1) v = (unsigned long long)__double_as_longlong(outlets[k].pour_level);
  reinterpret_cast<unsigned long long *>(t)[i] = v;
}

/* What a row block's kernels know beyond a whole raster's (kRows; wave-uniform all of it): the owned rows [ra, rb) of the view, over
 * which the strips are cut - neither pass has a stencil, so no row beyond them is ever read, not its dem and not its basins - and
 * the label -> slot table of the rims and catchments, through which the per-slot table is indexed. */
struct CurveRows {
  int ra, rb;
  const int *slot_of;
};

template <bool kRows>
__device__ __forceinline__ int curve_slot(const CurveRows &rw, int L) {
  return kRows ? rw.slot_of[L] : L - 1;
}

/* ---- bed ------------------------------------------------------------------------------------------------------------------- */
template <bool kRows>
__device__ __forceinline__ void curves_bed_body(const double *__restrict__ dem, const int *__restrict__ basins, const Geom &g, int rpw,
                                                int nwaves, CurveRow *table, const CurveRows &rw) {
  const int wid = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (wid >= nwaves) return;
  const int lane = threadIdx.x & 63;
  const int strip = wid / g.nsc, s = wid - strip * g.nsc;
  const int r0 = (kRows ? rw.ra : 0) + strip * rpw, r1 = min(r0 + rpw, kRows ? rw.rb : g.rows);
  const int c = s * kSeg + lane;
  const bool inside = c < g.ncp;
  int cy_label = 0;                        /* what the wave holds for one label and has not yet sent */
  unsigned long long cy_min = kNoBed;

  for (int r = r0; r < r1; r++) {
    const int b = inside ? basins[r * g.ncp + c] : -1;
    if (__ballot(b > 0) == 0ull) continue;
    const unsigned long long key = b > 0 ? depth_key(dem[r * g.ncp + c]) : kNoBed;
    /* per wave, by label */
    int cand = b > 0 ? b : 0;
    for (;;) {
      const unsigned long long pending = __ballot(cand != 0);
      if (pending == 0ull) break;
      const int L = __shfl(cand, __builtin_ctzll(pending));
      const unsigned long long lo = wave_min(cand == L ? key : kNoBed);
      if (cy_label != L) {                 /* down the rows: the same label goes on gathering, another one sends first */
        if (cy_label != 0 && lane == 0) atomic_min_if(&table[curve_slot<kRows>(rw, cy_label)].bed_key, cy_min);
        cy_label = L;
        cy_min = kNoBed;
      }
      cy_min = lo < cy_min ? lo : cy_min;
      if (cand == L) cand = 0;
    }
  }
  if (cy_label != 0 && lane == 0) atomic_min_if(&table[curve_slot<kRows>(rw, cy_label)].bed_key, cy_min);
}

__global__ __launch_bounds__(kBlock) void curves_bed_kernel(const double *__restrict__ dem, const int *__restrict__ basins, Geom g, int rpw,
                                                            int nwaves, CurveRow *table) {
  curves_bed_body<false>(dem, basins, g, rpw, nwaves, table, CurveRows());
}

/* the same over the owned rows of a row block's view: the rank's own lowest ground of every basin it holds cells of */
__global__ __launch_bounds__(kBlock) void curves_bed_rows_kernel(const double *__restrict__ dem, const int *__restrict__ basins, Geom g,
                                                                 int rpw, int nwaves, CurveRow *table, CurveRows rw) {
  curves_bed_body<true>(dem, basins, g, rpw, nwaves, table, rw);
}

/* ---- stages ---------------------------------------------------------------------------------------------------------------- */
/* what one lane holds for one label: its cells below every stage and their depths in quanta */
struct StageAcc {
  int label;                               /* 0: nothing held */
  unsigned n[kStages];
  unsigned long long q[kStages];
};

/* The lanes with `go` send what they hold: per wave by label, a butterfly sum per stage, lane 0 adds it to the pond's row.  Every
 * lane takes part in the exchanges. */
template <bool kRows>
__device__ __forceinline__ void stages_send(StageAcc &a, bool go, CurveRow *table, int lane, const CurveRows &rw) {
  int cand = go ? a.label : 0;
  for (;;) {
    const unsigned long long pending = __ballot(cand != 0);
    if (pending == 0ull) break;
    const int L = __shfl(cand, __builtin_ctzll(pending));
    const bool mine = cand == L;
    CurveRow *t = table + curve_slot<kRows>(rw, L);
#pragma unroll
    for (int s = 0; s < kStages; s++) {
      const unsigned cnt = wave_sum(mine ? a.n[s] : 0u);
      if (cnt != 0u) {                     /* wave-uniform */
        const unsigned long long sum = wave_sum(mine ? a.q[s] : 0ull);
        if (lane == 0) {
          atomicAdd(&t->cells[s], (unsigned long long)cnt);
          if (sum != 0ull) atomicAdd(&t->q[s], sum);
        }
      }
      if (mine) {
        a.n[s] = 0u;
        a.q[s] = 0ull;
      }
    }
    if (mine) {
      a.label = 0;
      cand = 0;
    }
  }
}

template <bool kRows>
__device__ __forceinline__ void curves_stages_body(const double *__restrict__ dem, const int *__restrict__ basins, const Geom &g, int rpw,
                                                   int nwaves, CurveRow *table, CurveStatus *st, const CurveRows &rw) {
  const int wid = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (wid >= nwaves) return;
  const int lane = threadIdx.x & 63;
  const int strip = wid / g.nsc, sc = wid - strip * g.nsc;
  const int r0 = (kRows ? rw.ra : 0) + strip * rpw, r1 = min(r0 + rpw, kRows ? rw.rb : g.rows);
  const int c = sc * kSeg + lane;
  const bool inside = c < g.ncp;
  int held = 0;                            /* the basin whose bed and top the lane holds */
  double bed = 0.0, top = 0.0;
  unsigned long long topkey = 0ull;
  StageAcc a;
  a.label = 0;
#pragma unroll
  for (int s = 0; s < kStages; s++) {
    a.n[s] = 0u;
    a.q[s] = 0ull;
  }
  bool bad = false;

  for (int r = r0; r < r1; r++) {
    const int b = inside ? basins[r * g.ncp + c] : -1;
    if (__ballot(b > 0) == 0ull) continue;
    if (b > 0 && b != held) {              /* every bed key is final: the bed pass has ended (over all ranks, for a row block) */
      const CurveRow *t = table + curve_slot<kRows>(rw, b);
      bed = depth_from_key(t->bed_key);
      top = t->top_level;
      topkey = depth_key(top);
      held = b;
    }
    const bool live = b > 0 && top < __builtin_inf();          /* a pond with an outlet: the pour level is finite or +inf */
    if (__ballot(live) == 0ull) continue;
    const double e = live ? dem[r * g.ncp + c] : 0.0;
    const unsigned long long ekey = depth_key(e);
    const bool wet = live && ekey < topkey;                     /* below the last stage, or below none */
    if (__ballot(wet) == 0ull) continue;
    const bool turn = wet && a.label != 0 && a.label != b;
    if (__ballot(turn) != 0ull) stages_send<kRows>(a, turn, table, lane, rw);
    if (wet) a.label = b;
#pragma unroll
    for (int s = 1; s <= kStages; s++) {
      const double h = s == kStages ? top : stage_between(bed, top, s);
      const double depth = h - e;
      const bool below = wet && ekey < depth_key(h);
      const bool ok = depth < 512.0;                            /* not 512 m or more, +inf, NaN */
      bad = bad || (below && !ok);
      if (below && ok) {
        a.n[s - 1] += 1u;
        a.q[s - 1] += (unsigned long long)rint(depth * 16777216.0);
      }
    }
  }
  stages_send<kRows>(a, a.label != 0, table, lane, rw);
  if (bad) st->deep = 1u;
}

__global__ __launch_bounds__(kBlock) void curves_stages_kernel(const double *__restrict__ dem, const int *__restrict__ basins, Geom g,
                                                               int rpw, int nwaves, CurveRow *table, CurveStatus *st) {
  curves_stages_body<false>(dem, basins, g, rpw, nwaves, table, st, CurveRows());
}

/* the same over the owned rows of a row block's view, against the bed keys the host merged over all ranks: a rank that holds cells of
 * a basin and not its bed forms the same sixteen heights as the rank that holds the bed */
__global__ __launch_bounds__(kBlock) void curves_stages_rows_kernel(const double *__restrict__ dem, const int *__restrict__ basins, Geom g,
                                                                    int rpw, int nwaves, CurveRow *table, CurveStatus *st, CurveRows rw) {
  curves_stages_body<true>(dem, basins, g, rpw, nwaves, table, st, rw);
}

/* ---- finish ---------------------------------------------------------------------------------------------------------------- */
/* the accumulated row becomes a wdpm_pond_curve in place; every lane stays for the counts */
__global__ __launch_bounds__(kBlock) void curves_finish_kernel(CurveRow *t, long long n, CurveStatus *st) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < n;
  bool none = false, flat = false;
  unsigned long long cells = 0ull;
  if (live) {
    const double bed = depth_from_key(t[i].bed_key), top = t[i].top_level;
    t[i].bed_key = (unsigned long long)__double_as_longlong(bed);
    none = !(top < __builtin_inf());
    flat = top == bed;
    cells = t[i].cells[kStages - 1];
  }
  const unsigned long long nonem = __ballot(none), flatm = __ballot(flat);
  cells = wave_sum(cells);
  if ((threadIdx.x & 63) == 0) {
    if (nonem) atomicAdd(&st->no_curve, (unsigned long long)__popcll(nonem));
    if (flatm) atomicAdd(&st->flat, (unsigned long long)__popcll(flatm));
    if (cells) atomicAdd(&st->stage_cells, cells);
  }
}

/* ---- row blocks: what goes between the ranks and the host -------------------------------------------------------------------- */
/* init over a rank's slots, one thread per 64-bit word as above.  The top level comes from the slot's outlet row as the group's outlet
 * pass left it on the device: its pour key is the one the host merged over all ranks (~0: no pass anywhere), so the double is the
 * merged table's pour_level bit for bit, +inf where the pond has no outlet. */
__global__ __launch_bounds__(kBlock) void curves_init_rows_kernel(CurveRow *t, long long n, const OutletRow *__restrict__ outlets) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n * kCurveWords) return;
  const long long k = i / kCurveWords;
  const int j = (int)(i - k * kCurveWords);
  unsigned long long v = 0ull;
  if (j == 0) v = kNoBed;
  if (j == 1) {
    const unsigned long long pour = outlets[k].pour_key;
    v = (unsigned long long)__double_as_longlong(pour == ~0ull ? __builtin_inf() : depth_from_key(pour));
  }
  reinterpret_cast<unsigned long long *>(t)[i] = v;
}

/* after the bed pass: every slot's bed key, side by side for one copy down.  The key stays a key: the host turns the lowest of all
 * ranks into a double, once per pond (wdpm_curves_merge.h). */
__global__ __launch_bounds__(kBlock) void curves_bed_down_kernel(const CurveRow *__restrict__ t, long long n, unsigned long long *__restrict__ out) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) out[i] = t[i].bed_key;
}

/* before the stage pass: every slot takes its pond's bed key as the host merged it over all ranks */
__global__ __launch_bounds__(kBlock) void curves_bed_up_kernel(CurveRow *__restrict__ t, long long n, const unsigned long long *__restrict__ keys) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) t[i].bed_key = keys[i];
}

}  // namespace

#ifndef WDPM_PONDS_EMULATION
/* ---- host ------------------------------------------------------------------------------------------------------------------ */
namespace {
const char kNoTable[] = "no curve table: the last label call on this handle was not a wdpm_curves_label that succeeded";
}  // namespace

extern "C" double wdpm_curves_stage_level(double bed, double top, int s) {
  if (s < 0 || s > kStages) return std::nan("");
  if (s == 0) return bed;
  if (s == kStages) return top;
  return stage_between(bed, top, s);
}

extern "C" int wdpm_curves_label(wdpm_ponds *h, double min_depth, int64_t *nponds) {
  if (!h) return wdpm_fail("wdpm_curves_label: null handle");
  if (check_min_depth("wdpm_curves_label", min_depth)) return 1;
  if (h->seams) return wdpm_fail("wdpm_curves_label: the handle views a row block: stage curves are taken on whole rasters only");
  int64_t n = 0;
  if (wdpm_outlets_label(h, min_depth, &n)) return 1;         /* leaves basin raster, outlet table and the stream as this pass wants them */
  h->lab.valid = false;                                       /* a wdpm_curves_label that fails leaves no table of any kind */
  wdpm_ctx *x = h->x;
  const Geom g = h->g;
  const hipStream_t sm = x->stream;
  HIP_TRY(hipSetDevice(x->p.device));
  const char *what;
  hipError_t e = ensure(h->cur.status, &what);
  if (e != hipSuccess) return wdpm_fail("wdpm_curves_label: no %s memory for the status words: %s", what, hipGetErrorString(e));
  e = grow(h, h->cur.table, n);                               /* sized from N, like the pond table */
  if (e != hipSuccess) return wdpm_fail("wdpm_curves_label: no device memory for the curves of %lld ponds: %s", (long long)n, hipGetErrorString(e));
  h->cur.timer.clear();
  memset(h->cur.status.h, 0, sizeof(CurveStatus));
  if (n > 0) {                                                /* no pond, no curve: nothing to launch */
    const double *dem = x->d_dem + (size_t)h->row_off * g.ncp;
    const Waves wv = waves_for(h, g.rows);
    const int rpw = wv.rpw, nwaves = wv.nwaves;
    const unsigned nblocks = blocks_for(n, kBlock), iblocks = blocks_for((long long)n * kCurveWords, kBlock), wblocks = blocks_for(nwaves, kWaves);
    const wdpm_pond_outlet *outlets = reinterpret_cast<const wdpm_pond_outlet *>(h->out.table.p);
    HIP_TRY(hipMemsetAsync(h->cur.status.d, 0, sizeof(CurveStatus), sm));
    HIP_TRY(h->cur.timer.mark(h->timing, 0, sm));
    hipLaunchKernelGGL(curves_init_kernel, dim3(iblocks), dim3(kBlock), 0, sm, h->cur.table.p, (long long)n, outlets);
    hipLaunchKernelGGL(curves_bed_kernel, dim3(wblocks), dim3(kBlock), 0, sm, dem, h->cat.link.p, g, rpw, nwaves, h->cur.table.p);
    HIP_TRY(h->cur.timer.mark(h->timing, 1, sm));
    hipLaunchKernelGGL(curves_stages_kernel, dim3(wblocks), dim3(kBlock), 0, sm, dem, h->cat.link.p, g, rpw, nwaves, h->cur.table.p, h->cur.status.d);
    hipLaunchKernelGGL(curves_finish_kernel, dim3(nblocks), dim3(kBlock), 0, sm, h->cur.table.p, (long long)n, h->cur.status.d);
    HIP_TRY(h->cur.timer.mark(h->timing, 2, sm));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->cur.status.h, h->cur.status.d, sizeof(CurveStatus), hipMemcpyDeviceToHost, sm));
    if (wdpm_stream_sync(x, sm)) return 1;
    if (h->timing) HIP_TRY(h->cur.timer.read_all());
  }
  if (h->cur.status.h->deep)
    return wdpm_fail("wdpm_curves_label: a cell of a pond's basin lies 512 m or more below a stage of the pond's curve, or not a finite "
                     "depth below it: q (64-bit sums of depths in units of 2^-24 m) is only safe below that depth");
  h->cur.stats.ponds = n;
  h->cur.stats.no_curve = (int64_t)h->cur.status.h->no_curve;
  h->cur.stats.flat = (int64_t)h->cur.status.h->flat;
  h->cur.stats.stage_cells = (int64_t)h->cur.status.h->stage_cells;
  h->cur.valid = true;
  h->lab.valid = true;
  if (nponds) *nponds = n;
  return 0;
}

extern "C" int wdpm_curves_table(wdpm_ponds *h, wdpm_pond_curve *out, int64_t capacity) {
  return table_out("wdpm_curves_table", h, &wdpm_ponds::cur, kNoTable, out, capacity);
}

extern "C" int wdpm_curves_stats(wdpm_ponds *h, wdpm_pond_curve_stats *out) {
  return stats_out("wdpm_curves_stats", h, &wdpm_ponds::cur, kNoTable, out);
}

extern "C" int wdpm_curves_phase_ms(wdpm_ponds *h, double *ms) {
  return phase_ms_out("wdpm_curves_phase_ms", h, &wdpm_ponds::cur, kNoTable, ms);
}

/* ---- row blocks (include/wdpm_group_pond_curves.h) --------------------------------------------------------------------------- */
#include "wdpm_curves_merge.h"

static_assert(sizeof(wdpm_curves_merge::SlotRow) == sizeof(CurveRow) && offsetof(wdpm_curves_merge::SlotRow, top_level) == offsetof(CurveRow, top_level) &&
              offsetof(wdpm_curves_merge::SlotRow, cells) == offsetof(CurveRow, cells) && offsetof(wdpm_curves_merge::SlotRow, q) == offsetof(CurveRow, q),
              "the merge reads the slots' rows as the device leaves them");

namespace {
const char kNoGroupTable[] = "no curve table: the last label call on this handle was not a wdpm_group_curves_label that succeeded";

CurveRows rows_of(const wdpm_group_ponds *gh, int i) {
  const OwnedRows own = owned_rows(gh, i);
  return {own.ra, own.rb, gh->r[i]->rim.slot_of.p};
}

/* rank i's buffers for `slots` table rows; nothing is queued */
int group_curves_buffers(wdpm_ponds *h, int i, long long slots) {
  HIP_TRY(hipSetDevice(h->x->p.device));
  const char *what;
  hipError_t e = ensure(h->cur.status, &what);
  if (e != hipSuccess) return wdpm_fail("wdpm_group_curves_label: no %s memory for the status words of rank %d: %s", what, i, hipGetErrorString(e));
  e = grow(h, h->cur.table, slots);
  if (e != hipSuccess) return wdpm_fail("wdpm_group_curves_label: no device memory for %lld curve rows of rank %d: %s", slots, i, hipGetErrorString(e));
  e = grow(h, h->cur.keys, slots);
  if (e != hipSuccess) return wdpm_fail("wdpm_group_curves_label: no device memory for the bed keys of %lld slots of rank %d: %s", slots, i, hipGetErrorString(e));
  e = grow(h, h->cur.h_keys, 2 * slots);
  if (e != hipSuccess) return wdpm_fail("wdpm_group_curves_label: no pinned host memory for the bed keys of %lld slots of rank %d: %s", slots, i, hipGetErrorString(e));
  e = grow(h, h->cur.h_table, slots);
  if (e != hipSuccess) return wdpm_fail("wdpm_group_curves_label: no pinned host memory for %lld curve rows of rank %d: %s", slots, i, hipGetErrorString(e));
  return 0;
}

/* one wait per rank that has work queued; the first message stays */
int group_curves_wait(wdpm_group_ponds *gh, int ev_a, int ev_b, int phase) {
  bool bad = false;
  std::string first_msg;
  for (int i = 0; i < gh->n; i++) {
    wdpm_ponds *p = gh->r[i];
    if (p->cat.slots == 0) continue;
    bool failed = hipSetDevice(p->x->p.device) != hipSuccess || wdpm_stream_sync(p->x, p->x->stream);
    if (!failed && p->timing) {
      const hipError_t e = p->cur.timer.read(ev_a, ev_b, &p->cur.timer.ms[phase]);
      if (e != hipSuccess) failed = wdpm_fail("wdpm_group_curves_label: the events of rank %d cannot be read: %s", i, hipGetErrorString(e)) != 0;
    }
    if (failed) {
      if (!bad) first_msg = wdpm_last_error();
      bad = true;
    }
  }
  return bad ? wdpm_fail("%s", first_msg.c_str()) : 0;
}
}  // namespace

extern "C" int wdpm_group_curves_label(wdpm_group_ponds *h, double min_depth, int64_t *nponds) {
  if (!h) return wdpm_fail("wdpm_group_curves_label: null handle");
  if (check_min_depth("wdpm_group_curves_label", min_depth)) return 1;
  int64_t n = 0;
  const int rc = wdpm_group_outlets_label(h, min_depth, &n);  /* leaves basins, slots and, in every slot's outlet row on the device, the merged pour key */
  h->lab.valid = false;                                       /* a wdpm_group_curves_label that fails leaves no table of any kind */
  if (rc) return 1;
  const int nr = h->n;
  for (int i = 0; i < nr; i++) {
    wdpm_ponds *p = h->r[i];
    p->cur.timer.clear();
    if (n > 0 && p->cat.slots > 0 && group_curves_buffers(p, i, p->cat.slots)) return 1;
  }
  h->cur.rows.resize((size_t)n);                              /* the merge writes every row */
  wdpm_curves_merge::Totals tot;
  long long split_basins = 0;
  double merge_ms = 0.0;
  if (n > 0) {                                                /* no pond, no curve: nothing to launch */
    /* (A) every rank: init, the bed pass over its owned rows, its slots' keys on their way down */
    for (int i = 0; i < nr; i++) {
      wdpm_ponds *p = h->r[i];
      if (p->cat.slots == 0) continue;                      /* no basin > 0 in its rows */
      wdpm_ctx *x = p->x;
      const Geom g = p->g;
      const hipStream_t sm = x->stream;
      const CurveRows rw = rows_of(h, i);
      const long long slots = p->cat.slots;
      const double *dem = x->d_dem + (size_t)p->row_off * g.ncp;
      const Waves wv = waves_for(p, rw.rb - rw.ra);
      const int rpw = wv.rpw, nwaves = wv.nwaves;
      hipError_t e = hipSetDevice(x->p.device);
      if (e == hipSuccess) e = hipMemsetAsync(p->cur.status.d, 0, sizeof(CurveStatus), sm);
      if (e == hipSuccess) e = p->cur.timer.mark(p->timing, 0, sm);
      if (e == hipSuccess) {
        hipLaunchKernelGGL(curves_init_rows_kernel, dim3(blocks_for(slots * kCurveWords, kBlock)), dim3(kBlock), 0, sm, p->cur.table.p, slots,
                           p->out.table.p);
        hipLaunchKernelGGL(curves_bed_rows_kernel, dim3(blocks_for(nwaves, kWaves)), dim3(kBlock), 0, sm, dem, p->cat.link.p, g, rpw, nwaves,
                           p->cur.table.p, rw);
        hipLaunchKernelGGL(curves_bed_down_kernel, dim3(blocks_for(slots, kBlock)), dim3(kBlock), 0, sm, p->cur.table.p, slots, p->cur.keys.p);
        e = hipGetLastError();
      }
      if (e == hipSuccess) e = p->cur.timer.mark(p->timing, 1, sm);
      if (e == hipSuccess) e = hipMemcpyAsync(p->cur.h_keys.p, p->cur.keys.p, (size_t)slots * sizeof(unsigned long long), hipMemcpyDeviceToHost, sm);
      if (e != hipSuccess) {
        (void)wdpm_fail("wdpm_group_curves_label: queueing the bed pass of rank %d failed: %s", i, hipGetErrorString(e));
        return group_drain(h);
      }
    }
    if (group_curves_wait(h, 0, 1, 0)) return 1;

    timespec t0, t1, t2, t3;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    std::vector<wdpm_curves_merge::Rank> ranks((size_t)nr);
    std::vector<unsigned long long *> up((size_t)nr);
    for (int i = 0; i < nr; i++) {
      const wdpm_ponds *p = h->r[i];
      wdpm_curves_merge::Rank &rk = ranks[(size_t)i];
      rk.label = p->rim.slot_label.data();
      rk.slots = p->cat.slots;
      rk.remote = p->cat.remote_label.data();
      rk.nremote = p->cat.remote;
      rk.key = p->cur.h_keys.p;
      rk.rows = reinterpret_cast<const wdpm_curves_merge::SlotRow *>(p->cur.h_table.p);
      up[(size_t)i] = p->cur.h_keys.p + p->cat.slots;           /* behind the slots words that came down */
    }
    std::vector<unsigned long long> bed_key((size_t)n);
    std::string err;
    if (wdpm_curves_merge::bed(ranks, n, bed_key.data(), up, split_basins, err)) return wdpm_fail("wdpm_group_curves_label: %s", err.c_str());
    clock_gettime(CLOCK_MONOTONIC, &t1);

    /* (B) every rank: the merged keys into its slots, the stage pass, its rows and its status word on their way down */
    for (int i = 0; i < nr; i++) {
      wdpm_ponds *p = h->r[i];
      if (p->cat.slots == 0) continue;
      wdpm_ctx *x = p->x;
      const Geom g = p->g;
      const hipStream_t sm = x->stream;
      const CurveRows rw = rows_of(h, i);
      const long long slots = p->cat.slots;
      const double *dem = x->d_dem + (size_t)p->row_off * g.ncp;
      const Waves wv = waves_for(p, rw.rb - rw.ra);
      const int rpw = wv.rpw, nwaves = wv.nwaves;
      hipError_t e = hipSetDevice(x->p.device);
      if (e == hipSuccess) e = p->cur.timer.mark(p->timing, 1, sm);
      if (e == hipSuccess) e = hipMemcpyAsync(p->cur.keys.p, up[(size_t)i], (size_t)slots * sizeof(unsigned long long), hipMemcpyHostToDevice, sm);
      if (e == hipSuccess) {
        hipLaunchKernelGGL(curves_bed_up_kernel, dim3(blocks_for(slots, kBlock)), dim3(kBlock), 0, sm, p->cur.table.p, slots, p->cur.keys.p);
        hipLaunchKernelGGL(curves_stages_rows_kernel, dim3(blocks_for(nwaves, kWaves)), dim3(kBlock), 0, sm, dem, p->cat.link.p, g, rpw, nwaves,
                           p->cur.table.p, p->cur.status.d, rw);
        e = hipGetLastError();
      }
      if (e == hipSuccess) e = p->cur.timer.mark(p->timing, 2, sm);
      if (e == hipSuccess) e = hipMemcpyAsync(p->cur.h_table.p, p->cur.table.p, (size_t)slots * sizeof(CurveRow), hipMemcpyDeviceToHost, sm);
      if (e == hipSuccess) e = hipMemcpyAsync(p->cur.status.h, p->cur.status.d, sizeof(CurveStatus), hipMemcpyDeviceToHost, sm);
      if (e != hipSuccess) {
        (void)wdpm_fail("wdpm_group_curves_label: queueing the stage pass of rank %d failed: %s", i, hipGetErrorString(e));
        return group_drain(h);
      }
    }
    if (group_curves_wait(h, 1, 2, 1)) return 1;
    for (int i = 0; i < nr; i++)
      if (h->r[i]->cat.slots > 0 && h->r[i]->cur.status.h->deep)
        return wdpm_fail("wdpm_group_curves_label: a cell of a pond's basin lies 512 m or more below a stage of the pond's curve, or not a finite "
                         "depth below it: q (64-bit sums of depths in units of 2^-24 m) is only safe below that depth");

    clock_gettime(CLOCK_MONOTONIC, &t2);
    if (wdpm_curves_merge::merge(ranks, n, bed_key.data(), h->cur.rows.data(), tot, err)) return wdpm_fail("wdpm_group_curves_label: %s", err.c_str());
    clock_gettime(CLOCK_MONOTONIC, &t3);
    merge_ms = ms_between(t0, t1) + ms_between(t2, t3);
  }
  h->cur.stats.ponds = n;
  h->cur.stats.no_curve = tot.no_curve;
  h->cur.stats.flat = tot.flat;
  h->cur.stats.stage_cells = tot.stage_cells;
  h->cur.stats.ranks = nr;
  h->cur.stats.split_basins = split_basins;
  h->cur.stats.remote_beds = tot.remote_beds;
  h->cur.stats.merge_ms = merge_ms;
  h->cur.valid = true;
  h->lab.valid = true;
  if (nponds) *nponds = n;
  return 0;
}

extern "C" int wdpm_group_curves_table(wdpm_group_ponds *h, wdpm_pond_curve *out, int64_t capacity) {
  return table_out("wdpm_group_curves_table", h, &wdpm_group_ponds::cur, kNoGroupTable, out, capacity);
}

extern "C" int wdpm_group_curves_stats(wdpm_group_ponds *h, wdpm_group_curve_stats *out) {
  return stats_out("wdpm_group_curves_stats", h, &wdpm_group_ponds::cur, kNoGroupTable, out);
}

extern "C" int wdpm_group_curves_phase_ms(wdpm_group_ponds *h, int32_t rank, double *ms) {
  return group_phase_ms_out("wdpm_group_curves_phase_ms", h, &wdpm_group_ponds::cur, &wdpm_ponds::cur, kNoGroupTable, rank, ms);
}
#endif  /* WDPM_PONDS_EMULATION */
