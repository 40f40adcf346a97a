/*
 * wdpm_march.hip — the marching kernel (fused_iteration_kernel) and the launch of an iteration: each raster read from HBM once, the
 * water raster written once, 24 B per cell-update, the algorithmic minimum.  What it shares with the kernels of
 * small rasters (wdpm_small.hip) - the trapezoid, the lane layout, the DPP borrow, the per-block arithmetic - is wdpm_iteration.h.
 * This unit is built under the compiler's max-ILP instruction scheduler (Makefile; why: wdpm_small.hip).
 *
 *  - Waves never synchronise with each other (no barriers; LDS is only a wave-private transpose buffer for the stores).
 *    Waves per SIMD: two wherever chunks of 18 (add / subtract on the DEM codes) or 12 rows
 *    (drain) fill every slot, one otherwise.  With two, a workgroup is eight waves and the two waves of a SIMD tell each other
 *    their step through LDS: whoever is behind is served first (see the marching loop).  Chunk heights follow what each XCD
 *    delivers (wdpm_kernels.h::XcdBalance).  Round 4's counters: fp64 VALU issue in ~89 % of the kernel's cycles, ~4.7 TB/s of
 *    HBM traffic - between both ceilings.
 *  - The wave marches down a chunk of rows with a 7-row window held in registers (dem + water,
 *    3 columns per lane).  Each step loads 3 new rows and applies, in this order, row alignment
 *    oi=1 to rows 3n..3n+2, oi=2 to rows 3n-2..3n, oi=3 to rows 3n-4..3n-2.  Rows 3n-4..3n-2 are then final
 *    and are stored.
 *  - DEM32: the static DEM can be streamed as 32-bit codes q with dem == (q + k0) / 10^e bit for bit
 *    (verified per cell at upload by the decoder used here, wdpm_stencil.h::dem32_decode): 12 bytes
 *    per lane and row in one global_load_dwordx3, 20 B of HBM traffic per cell-update instead of 24 - on the largest launches
 *    as 16-bit offsets from one 32-bit base per 48 columns (18.1 B; wdpm_kernels.h::DemCode).
 *  - Memory operations are unconditional and fixed in number per step (prefetch by inline-asm
 *    loads one step ahead, exact s_waitcnt; stores transposed through LDS to 512-byte contiguous
 *    writes, saddr-form inline asm, issued at the top of the following step).
 *  - The neighbour step is 9 (add) / 14 (drain) VALU instructions where the depths a wave holds allow the one-instruction
 *    clamped max(x / 8, -0.0) (wdpm_stencil.h; `deep` below), 10 / 15 otherwise.
 *
 * The marching kernel has two loops: its own, and iter2_march for launches that run two iterations (producer and consumer waves).
 * What a step of either does with its rows - the lane offsets, the inline-asm prefetch and its exact wait, the decode into the
 * window, the edge mask, `deep`, the staged stores, the window slide - is written once, in the functions in front of iter2_march;
 * the loops themselves hold what is theirs alone.  Behind the kernels: the balance kernel (xcd_rebalance_kernel), the DPP probe
 * (dpp_probe_kernel, dpp_selfcheck), the device facts and wdpm_launch_iteration, which queues what plan_iteration decided and
 * hands the plans of small rasters to wdpm_launch_small.
 */
#include "wdpm_iteration.h"

#include <atomic>
#include <mutex>
#include <type_traits>

namespace {

/* Drain: the outlet branch of runoffd() costs ten more instructions per neighbour step, and exactly
 * one cell of the raster needs it.  Whether any of the seven rows of this step's window is the outlet's
 * row is wave-uniform (computed on the scalar unit), so all other steps run the plain neighbour step -
 * as ONE basic block of three stages, which lets the scheduler overlap the stages' tails and heads
 * (a test per stage cut the step into three blocks). */
/* NSTAGES < 3: the first two steps of a chunk.  Step 0 holds real rows only in slots 4..6: its oi = 2 block has its centre
 * on an empty slot (dem = +inf: nothing moves), its oi = 3 block lies on empty slots altogether.  Step 1's oi = 3 block
 * (rows A-1 .. A+1, centre row A) touches rows A and A+1 only, after the last pass that reads them in this iteration, and
 * those rows are never stored (a chunk stores from row A+2; for A = 0 the centre row is the raster's border or a slab's
 * first halo row, which is wrong from the first iteration after a refresh on anyway): dead work.  Leaving those three stage
 * executions out saves 3 of 3 (H/3 + 2): 9 % of a 27-row chunk, 5.6 % at 48 rows, 0.4 % at 780. */
template <int MODULE, bool SZ_SAFE, int NSTAGES = 3, int PLAIN = 0>
__device__ __forceinline__ void three_stages(double (&W)[7][3], const double (&D)[7][3], const int rbase,
                                             const int drain_row, const bool (&cdr)[5], DrainState &ds) {
  if (MODULE == 2 && drain_row >= rbase && drain_row <= rbase + 6) {           // wave-uniform, rare
    stage_impl<MODULE, SZ_SAFE, 4, true>(W, D, rbase + 4, drain_row, cdr, ds);   // oi = 1 on rows 3n   .. 3n+2
    if (NSTAGES >= 2) stage_impl<MODULE, SZ_SAFE, 2, true>(W, D, rbase + 2, drain_row, cdr, ds);   // oi = 2 on rows 3n-2 .. 3n
    if (NSTAGES >= 3) stage_impl<MODULE, SZ_SAFE, 0, true>(W, D, rbase + 0, drain_row, cdr, ds);   // oi = 3 on rows 3n-4 .. 3n-2
  } else {
    stage_impl<MODULE, SZ_SAFE, 4, false, PLAIN>(W, D, rbase + 4, drain_row, cdr, ds);
    if (NSTAGES >= 2) stage_impl<MODULE, SZ_SAFE, 2, false, PLAIN>(W, D, rbase + 2, drain_row, cdr, ds);
    if (NSTAGES >= 3) stage_impl<MODULE, SZ_SAFE, 0, false, PLAIN>(W, D, rbase + 0, drain_row, cdr, ds);
  }
}

#ifdef WDPM_WAVE_TIMES   /* timing builds only (tools/wave_times.py): when each wave of the marching kernel starts and ends, and where */
static __device__ unsigned long long g_wave_times[4 * 8192];   /* this unit's own (wdpm_small.hip has one for the relay kernel): each has its accessor */
/* two-iteration launches: what each wave spent in await(), by where in its chunk (start: steps 0 - 3, end: the last four, steady between).
 * A producer only ever waits for a full ring, a consumer for an empty one.  Per wave: [0] polls start | steady << 32, [1] polls end |
 * awaits that had to poll << 32, [2] 100 MHz ticks from first poll to release, start | steady << 32, [3] the same at the end */
static __device__ unsigned long long g_wave_waits[4 * 8192];
#endif
#ifndef WDPM_FUSED_MIN_WAVES
#define WDPM_FUSED_MIN_WAVES 2   /* waves per SIMD the register allocator must leave room for */
#endif
#ifndef WDPM_FUSED_CODES_WAVES
#define WDPM_FUSED_CODES_WAVES 2 /* the same for the add / subtract instances that stream the DEM as codes */
#endif

/* raw registers of the row prefetch.  DEM32: the dem rows arrive as 32-bit codes, a lane's three columns
 * in one 12-byte load (qi).  Only the members an instantiation uses exist. */
typedef int wdpm_i3 __attribute__((ext_vector_type(3)));
struct Prefetched {
  double NW[3][3], ND[3][3];
  wdpm_i3 qi[3];
  int qh[3][3];      /* DEM32 == 2: 16-bit offsets (zero-extended by the load) ... */
  int gbv[3];        /* ... and the lane's group base per row */
};

/* waves per SIMD an instantiation is built for.  The drain variant for rasters that hold a -0.0 depth (SZ_SAFE: the reference's
 * conditional 21-instruction step) does not fit two waves' 256 VGPRs - it spilled 12 bytes in round 3 - and is built for one. */
template <int MODULE, bool SZ_SAFE, int DEM32, bool MD>
constexpr int fused_built_for() {
  return (MODULE == 2 && SZ_SAFE) ? 1 : (MODULE != 2 && DEM32 != 0 && !MD && !SZ_SAFE) ? WDPM_FUSED_CODES_WAVES : WDPM_FUSED_MIN_WAVES;
}

/* ---------------------------------------------------------------------------------------------
 * The parts of a marching step that the single loop (fused_iteration_kernel) and the loop of two-iteration launches (iter2_march)
 * share - one implementation, templated on what differs: DEM32 (0 / 1 / 2), EDGE (a wave that can touch cells outside the slab) and
 * WATER (the water rows come from memory: the single loop and a two-iteration producer; a consumer takes them out of the ring).
 * A step of either loop keeps this order: the new rows' loads issued (prefetch_rows), the previous step's stores behind them
 * (StoreSide::write_staged), the stages, the wait for the loads (wait_rows), the slide (slide_window).
 * --------------------------------------------------------------------------------------------- */

/* lane byte offsets inside a row: interior waves use one offset + immediates, edge waves clamp
 * every column into the raster (values of clamped cells are masked on use) */
/* Edge waves clamp the row (scalar) and the lane's first column into the raster and read their three columns with the same
 * one-offset loads as everybody else: a lane whose columns straddle the row's end reads up to two cells past it - the next
 * row's first cells, or, in the slab's last row, the 192 spare cells behind every raster wdpm_create allocates (16 codes behind
 * the DEM codes) - and masks them on use, as it masks whole lanes beyond the raster.  (Rounds 1 - 3 clamped column by column:
 * nine loads per row instead of three, and the edge waves were the last of every launch to end, round 4.) */
struct RowOffsets {
  int voff0;     // the lane's first column in an 8-byte raster row; loop-invariant: the clamp costs the interior waves nothing
  int qoff0;     // the same for the 4-byte dem codes,
  int hoff0;     // the 2-byte offsets
  int goff0;     // and the 4-byte group bases (one per kDemGroup columns)
  __device__ __forceinline__ RowOffsets(const int colb, const int ncp)
      : voff0(8 * (colb < ncp ? colb : ncp - 1)), qoff0(voff0 / 2), hoff0(voff0 / 4), goff0(4 * ((voff0 / 8) / kDemGroup)) {}
};

/* Prefetch of the three rows starting at r0 into raw registers.  The loads are issued with
 * inline asm (saddr form: wave-uniform row base in SGPRs + a per-lane byte offset) so that
 * they stay exactly here, one whole step ahead of their use, and are waited for with an exact
 * `s_waitcnt vmcnt(9)` (the 9 stores of the step are the only younger memory operations).
 * Left to the compiler the loads get sunk next to their consumer or guarded by vmcnt(0), which
 * exposes a full memory round trip per step.  The registers are not read before wait_rows().
 * `dem` is read only where DEM32 == 0. */
template <int DEM32, bool EDGE, bool WATER>
__device__ __forceinline__ void prefetch_rows(Prefetched &P, const int r0, const RowOffsets &o, const double *__restrict__ win,
                                              const double *__restrict__ dem, const DemCode &code, const SlabGeom g) {
  const size_t pitch = (size_t)g.ncp;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    int r = r0 + i;
    if (EDGE) r = r < g.rows ? r : g.rows - 1;
#ifdef WDPM_ABLATE_HBM   /* timing experiments only (tools/build_variant.sh ablateN -DWDPM_ABLATE_HBM=N, then tools/ab_interleaved.sh): what the kernel costs when its rows come from / go to the caches
                            instead of HBM.  Bits: 1 = the water loads come from the raster's first 48 rows, 2 = the stores land there,
                            4 = the DEM loads come from there.  Same instructions, same number of memory operations, wrong results. */
    const int rw = (WDPM_ABLATE_HBM & 1) ? r % 48 : r, rdm = (WDPM_ABLATE_HBM & 4) ? r % 48 : r;
#else
    const int rw = r, rdm = r;
#endif
    if (WATER) {
      const double *bw = win + (size_t)rw * pitch;     // wave-uniform, as every row base
      asm volatile("global_load_dwordx2 %0, %1, %2" : "=v"(P.NW[i][0]) : "v"(o.voff0), "s"(bw) : "memory");
      asm volatile("global_load_dwordx2 %0, %1, %2 offset:8" : "=v"(P.NW[i][1]) : "v"(o.voff0), "s"(bw) : "memory");
      asm volatile("global_load_dwordx2 %0, %1, %2 offset:16" : "=v"(P.NW[i][2]) : "v"(o.voff0), "s"(bw) : "memory");
    }
    if (DEM32 == 2) {
      const unsigned short *bh = code.h + (size_t)rdm * pitch;
      const int *bg = code.gb + (size_t)rdm * code.ngroups;
      asm volatile("global_load_ushort %0, %1, %2" : "=v"(P.qh[i][0]) : "v"(o.hoff0), "s"(bh) : "memory");
      asm volatile("global_load_ushort %0, %1, %2 offset:2" : "=v"(P.qh[i][1]) : "v"(o.hoff0), "s"(bh) : "memory");
      asm volatile("global_load_ushort %0, %1, %2 offset:4" : "=v"(P.qh[i][2]) : "v"(o.hoff0), "s"(bh) : "memory");
      asm volatile("global_load_dword %0, %1, %2" : "=v"(P.gbv[i]) : "v"(o.goff0), "s"(bg) : "memory");
    } else if (DEM32) {
      const int *bq = code.q + (size_t)rdm * pitch;
      asm volatile("global_load_dwordx3 %0, %1, %2" : "=v"(P.qi[i]) : "v"(o.qoff0), "s"(bq) : "memory");
    } else {
      const double *bd = dem + (size_t)rdm * pitch;
      asm volatile("global_load_dwordx2 %0, %1, %2" : "=v"(P.ND[i][0]) : "v"(o.voff0), "s"(bd) : "memory");
      asm volatile("global_load_dwordx2 %0, %1, %2 offset:8" : "=v"(P.ND[i][1]) : "v"(o.voff0), "s"(bd) : "memory");
      asm volatile("global_load_dwordx2 %0, %1, %2 offset:16" : "=v"(P.ND[i][2]) : "v"(o.voff0), "s"(bd) : "memory");
    }
  }
}

/* the wait that makes the prefetched registers readable; every register is an in/out operand so
 * no use can be scheduled above it.  YOUNGER = memory operations issued after the loads, counted exactly: 0, or the 9 stores of a
 * step (a two-iteration producer issues no memory operation behind its loads, a consumer its nine stores). */
template <int DEM32, bool WATER, int YOUNGER>
__device__ __forceinline__ void wait_rows(Prefetched &P) {
#define WDPM_ROWS_W "+v"(P.NW[0][0]), "+v"(P.NW[0][1]), "+v"(P.NW[0][2]), "+v"(P.NW[1][0]), "+v"(P.NW[1][1]), \
                    "+v"(P.NW[1][2]), "+v"(P.NW[2][0]), "+v"(P.NW[2][1]), "+v"(P.NW[2][2])
#define WDPM_ROWS_D "+v"(P.ND[0][0]), "+v"(P.ND[0][1]), "+v"(P.ND[0][2]), "+v"(P.ND[1][0]), "+v"(P.ND[1][1]), \
                    "+v"(P.ND[1][2]), "+v"(P.ND[2][0]), "+v"(P.ND[2][1]), "+v"(P.ND[2][2])
#define WDPM_ROWS_H "+v"(P.qh[0][0]), "+v"(P.qh[0][1]), "+v"(P.qh[0][2]), "+v"(P.qh[1][0]), "+v"(P.qh[1][1]), "+v"(P.qh[1][2]), \
                    "+v"(P.qh[2][0]), "+v"(P.qh[2][1]), "+v"(P.qh[2][2]), "+v"(P.gbv[0]), "+v"(P.gbv[1]), "+v"(P.gbv[2])
#define WDPM_ROWS_Q "+v"(P.qi[0]), "+v"(P.qi[1]), "+v"(P.qi[2])
#define WDPM_WAIT_ROWS(...) asm volatile("s_waitcnt vmcnt(%[younger])" : __VA_ARGS__ : [younger] "n"(YOUNGER) : "memory")
  static_assert(WATER || DEM32 != 0, "a wave that loads neither water nor DEM rows has nothing to wait for");
  if constexpr (WATER && DEM32 == 0) WDPM_WAIT_ROWS(WDPM_ROWS_W, WDPM_ROWS_D);
  else if constexpr (WATER && DEM32 == 2) WDPM_WAIT_ROWS(WDPM_ROWS_W, WDPM_ROWS_H);
  else if constexpr (WATER) WDPM_WAIT_ROWS(WDPM_ROWS_W, WDPM_ROWS_Q);
  else if constexpr (DEM32 == 2) WDPM_WAIT_ROWS(WDPM_ROWS_H);
  else WDPM_WAIT_ROWS(WDPM_ROWS_Q);
#undef WDPM_WAIT_ROWS
#undef WDPM_ROWS_Q
#undef WDPM_ROWS_H
#undef WDPM_ROWS_D
#undef WDPM_ROWS_W
}

/* "does any lane hold a NODATA offset (0xFFFF) in these three rows?" - the loads zero-extend, so the maximum of the nine says it.
 * Wave-uniform, the pattern of any_above_3m: four v_max3_u32, one compare, one scalar branch. */
__device__ __forceinline__ bool any_nodata16(const int (*h)[3]) {
  auto max3 = [](const unsigned a, const unsigned b, const unsigned c) { const unsigned m = a > b ? a : b; return m > c ? m : c; };
  unsigned hm = max3((unsigned)h[0][0], (unsigned)h[0][1], (unsigned)h[0][2]);
  hm = max3(hm, (unsigned)h[1][0], (unsigned)h[1][1]);
  hm = max3(hm, (unsigned)h[1][2], (unsigned)h[2][0]);
  hm = max3(hm, (unsigned)h[2][1], (unsigned)h[2][2]);
  return __ballot(hm >= 0xFFFFu) != 0;
}

/* consume the prefetched rows into window slots 4..6; the device DEM already holds +inf for
 * NODATA cells, so only edge waves have anything to mask (mask_outside) */
template <int DEM32, bool FLUSH>
__device__ __forceinline__ void decode_rows(double (&W)[7][3], double (&D)[7][3], const Prefetched &P, const DemCode &code, const double thres) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      // FLUSH: the block's threshold flush (WDPMCL.c:1059-1062) applied to the water as it arrives
      W[4 + i][j] = FLUSH && P.NW[i][j] < thres ? 0.0 : P.NW[i][j];
      if (DEM32 == 2) continue;
      else if (DEM32) D[4 + i][j] = dem32_decode_nan(P.qi[i][j], code.k0, code.D, code.rD, code.rDlo);
      else D[4 + i][j] = P.ND[i][j];
    }
  if (DEM32 == 2) {
    /* 16-bit offsets: a step whose wave holds no NODATA offset - every step of a raster without NODATA, and of real DEMs all steps
     * inside the basin - leaves the nine compares and selects out: 24 VALU instructions fewer on that path, the test included
     * (a two-iteration producer's step: 1658 -> 1634; profiles/r21/isa_loop_stats.txt).  One scalar branch per step, no new instantiation; a wave that does hold one (an edge lane's
     * clamped columns count) runs the full form on all nine.  16384^2, a block of 1000: -2.2 % and -3.0 % in two interleaved
     * sessions (profiles/r21/README.md). */
    if (any_nodata16(P.qh)) {
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) D[4 + i][j] = dem16_decode_nan<false>(P.qh[i][j], P.gbv[i], code.k0, code.D, code.rD, code.rDlo);
    } else {
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) D[4 + i][j] = dem16_decode_nan<true>(P.qh[i][j], P.gbv[i], code.k0, code.D, code.rD, code.rDlo);
    }
  }
}

/* edge waves: cells of window slots 4..6 (slab rows r0 .. r0 + 2) outside the slab hold dem = +inf, w = 0 */
__device__ __forceinline__ void mask_outside(double (&W)[7][3], double (&D)[7][3], const int r0, const int colb, const SlabGeom g) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const bool row_ok = r0 + i < g.rows;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const bool ok = row_ok & (colb + j < g.ncp);
      W[4 + i][j] = ok ? W[4 + i][j] : 0.0;
      D[4 + i][j] = ok ? D[4 + i][j] : WDPM_INF;
    }
  }
}

/* CLAMP (round 4; wdpm_stencil.h::eighth_clamped): one instruction less per neighbour step, exact while no flow of the step
 * exceeds 1 m.  A flow is at most (the centre's depth + half an ulp of its elevation) / 8, a cell receives in at most eight
 * of an iteration's nine passes (it is the centre of the ninth), and within one pass in at most one block: if every depth of
 * the window was <= M when it was loaded, every depth the window holds during the iteration is <= M (9/8)^8 + 8 ulp < 2.566 M + 8 ulp.
 * With M < 3.000002 m (any_above_3m on the nine values a step loads) and elevations below 2^30 m in magnitude (the host's part:
 * `no_clamp`) that is < 7.7 m.  The seven rows of a step's window were loaded by this step and the two before it: bits 0..2 of
 * `deep`; bit 3 = no_clamp.  A step with any of them set runs the unclamped stages - same results, the round-3 instruction
 * count.  Wave-uniform: one scalar branch per step. */
__device__ __forceinline__ int deep_next(const int deep, const double (&W)[7][3]) {
  return (deep & 8) | ((deep & 3) << 1) | (any_above_3m(&W[4]) ? 1 : 0);
}

/* slide the window down three rows */
__device__ __forceinline__ void slide_window(double (&W)[7][3], double (&D)[7][3]) {
#pragma unroll
  for (int k = 0; k < 4; k++)
#pragma unroll
    for (int j = 0; j < 3; j++) { W[k][j] = W[k + 3][j]; D[k][j] = D[k + 3][j]; }
}

/* Store side of a marching wave: after the LDS transpose, store instruction k = 0,1,2 writes the strip-relative
 * columns lo + 64k + lane of the exact output range [lo, hi].  Lanes past hi are clamped to hi:
 * they read the same LDS word and write the same address with the same value as the last valid
 * lane, so every store is unconditional (fixed instruction count) and nothing is written twice
 * with different data. */
struct StoreSide {
  double *wout;
  // Cells a wave must not write (outside its exact output block) are redirected to a 64-double
  // dump area behind the raster instead of being branched around: the loop then issues the same
  // number of loads and stores on every trip, so the compiler can wait with exact vmcnt counts
  // (with conditional memory operations it falls back to vmcnt(0) at the top of each step, which
  // exposes the full latency of the stores just issued — measured 27 % of the kernel).
  // (192 doubles behind the raster, allocated by wdpm_create: a dumped row goes there at the same lane offsets as a stored one, so
  // that every store is "uniform base + lane offset" - the saddr form, no 64-bit address arithmetic on the vector unit: nine
  // v_lshl_add_u64 per step less, round 4)
  char *dump;
  size_t pitch;
  int c0;                 // the strip's first column
  int or_lo, or_hi;       // the slab rows this wave stores
  bool any;               // false: nothing of this strip is stored (a two-iteration consumer whose strip lies beyond the raster)
  int scol[3];
  unsigned soff[3];       // the same as byte offsets: a store's address is a wave-uniform row base (SGPRs) + this

  __device__ __forceinline__ StoreSide(double *const wout_, const SlabGeom g, const int c0_, const int or_lo_, const int or_hi_)
      : wout(wout_), dump(reinterpret_cast<char *>(wout_ + (size_t)g.rows * g.ncp)), pitch((size_t)g.ncp), c0(c0_), or_lo(or_lo_),
        or_hi(or_hi_), any(true) {}
  /* [lo, hi]: the strip-relative columns of the exact output range */
  __device__ __forceinline__ void columns(const int lo, const int hi, const int lane) {
#pragma unroll
    for (int k = 0; k < 3; k++) { scol[k] = lo + 64 * k + lane < hi ? lo + 64 * k + lane : hi; soff[k] = 8u * (unsigned)scol[k]; }
  }
  // the three staged rows [rb, rb+2] from LDS to HBM: 9 unconditional stores.  In two halves: the LDS reads go out at
  // the very top of a step, ahead of the decode work, so that their round trip is over when the stores want the values
  // (issued right in front of the stores, each step stalled on it: +0.4 % at 8192^2, profiles/r02/early_lds_ab.txt)
  __device__ __forceinline__ void read_staged(double (&staged)[3][3], const double *stage_lds) const {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int k = 0; k < 3; k++) staged[i][k] = stage_lds[i * kStripIn + scol[k]];
  }
  __device__ __forceinline__ void write_staged(const double (&staged)[3][3], const int rb) const {
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const int r = rb + i;
      const bool row_ok = r >= or_lo && r <= or_hi && any;       // wave-uniform
      // rows outside the chunk's output range (first / last trips only) go to the dump area
#ifdef WDPM_ABLATE_HBM
      char *const orow = row_ok ? reinterpret_cast<char *>(wout + (size_t)((WDPM_ABLATE_HBM & 2) ? r % 48 : r) * pitch + c0) : dump;
#else
      char *const orow = row_ok ? reinterpret_cast<char *>(wout + (size_t)r * pitch + c0) : dump;   // wave-uniform
#endif
      // Stores as inline asm, saddr form: a wave-uniform row base in SGPRs + the lane's byte offset, no address arithmetic on
      // the vector unit.  Ordinary stores, not non-temporal ones (round 4).  Rounds 1 - 3 believed they were choosing between
      // the two by size: left to the compiler, the two arms of that branch (the same store with and without !nontemporal)
      // had been merged into ONE plain store with a 64-bit VALU address - round 3's final ISA has no `nt` store in this
      // kernel at all.  With real `nt` stores measured against plain ones (profiles/r04/stores_shapes_ab.txt): add 4096^2
      // 108.0 against 103.1 us, 3000^2 65.9 against 62.9, drain 8192^2 401.6 against 397.8, the 1053-row drain slab 77.7
      // against 75.2; a tie at 8192^2 add, on the 2116-row add slab and at 16384^2; drain 4096^2 128.9 against 130.3.
#pragma unroll
      for (int k = 0; k < 3; k++) asm volatile("global_store_dwordx2 %0, %1, %2" : : "v"(soff[k]), "v"(staged[i][k]), "s"(orow) : "memory");
    }
    __builtin_amdgcn_wave_barrier();
  }
};

/* ---------------------------------------------------------------------------------------------
 * Two iterations per launch (Iter2Args; geometry: wdpm_dispatch.h::plan_iter2).  A second marching loop of the gate-free add /
 * subtract instantiations that stream the DEM as codes, chosen by a kernel argument.
 *
 * A workgroup takes a GROUP of four neighbouring strips (kGroupIn = 705 columns in) and one chunk of rows.  Waves 0 - 3 are
 * producers: today's loop on iteration k, strip j = wave, from one row triple above the chunk (sh) to two below it - but the rows a
 * step finishes go into a ring of group rows in LDS instead of to memory, each producer depositing its exact columns (the group's
 * outer producers also their halo, so that every ring cell holds a finite value).  Waves 4 - 7 are consumers: today's loop on iteration
 * k + 1, strip j = wave - 4, whose water rows come out of the ring - all 192 columns of a consumer's strip lie in the ring row,
 * exact except for the group's outer 8 / 13 columns - and whose DEM codes come from memory as before (an L2 hit behind the
 * producer).  The group stores the 663 columns that are exact after both iterations (kGroupOut: all but 17 on the left and 25 on
 * the right, wdpm_dispatch.h); groups tile the raster.
 *
 * Hand-over: one word per wave in LDS (hand[]).  A producer's word counts the steps whose rows it has deposited, a consumer's the
 * row triples it has taken out of the ring.  Consumer triple t (rows 3t .. 3t+2 of the chunk) is complete after producer step
 * t + 2 + sh/3 of its own producer and of its neighbours; a producer's step n overwrites what consumer triple n - sh/3 - R/3 - 1
 * read.  A wave's LDS operations are carried out in order, so a word written behind the data (read behind the taking) needs no wait
 * of its own.  Waits are s_sleep polls and BOUNDED: a wave that runs out sets Iter2Args::err, stops waiting for the rest of
 * the launch (results are then wrong, the host fails the call) and the launch ends.  Producers wait for consumers only when the
 * ring is full and consumers for producers only when it is empty, consumers always behind: no cycle.  Roles follow from the
 * wave index alone; nothing depends on which SIMD a wave sits on.
 * --------------------------------------------------------------------------------------------- */
constexpr int kIter2Polls = 1 << 21;     /* of ~0.15 us each: a quarter of a second, against steps of a microsecond */
constexpr int kIter2Retired = 1 << 30;   /* hand word of a wave that has left: above every step count, far from overflow in `n - lag - taken` */

template <int DEM32>
__device__ __forceinline__ void iter2_march(const double *__restrict__ win, double *__restrict__ wout, const DemCode &code, const SlabGeom &g,
                                            const int H, const int out_last, const int no_clamp, const BalanceArgs &bal, const Iter2Args &i2,
                                            const int vb, const int wave, const int lane, const int share, const int xcc_phys,
                                            double *const stage_lds) {
  extern __shared__ double i2_ring[];                     // (ring_rows + 1) x kRingPitch
  __shared__ int hand[8];
  if (threadIdx.x < 8) hand[threadIdx.x] = 0;
  __syncthreads();
  if (vb >= i2.ngroups * i2.nchunks) return;              // workgroup-uniform
#ifdef WDPM_WAVE_TIMES
  const unsigned long long wt0 = wall_clock64();
#endif
  const int grp = vb % i2.ngroups, chunk = vb / i2.ngroups;
  const bool producer = wave < 4;                         // wave-uniform (SGPRs), as everything derived from it
  const int j = wave & 3;
  const int c0 = kGroupOut * grp + kStripOut * j;
  int A = H * chunk, A_next = A + H;
  if (bal.table) {                                        // row boundaries per group (see the single loop): all four strips share them
    A = bal.table[chunk * i2.ngroups + grp];
    A_next = bal.table[(chunk + 1) * i2.ngroups + grp];
    A = A < 0 ? 0 : (A > g.rows ? g.rows : A);
    A = A / 3 * 3;
    const int h = A_next - A;
    A_next = A + (h < 3 ? 3 : (h > 30000 ? 30000 : h)) / 3 * 3;
  }
  const unsigned long long bal_t0 = bal.acc ? wall_clock64() : 0;
  const int sh = A >= 3 ? 3 : 0;                          // the producer starts a row triple above the chunk (none above the raster)
  const int lag = 2 + sh / 3;                             // consumer triple t needs producer step t + lag
  const int NC = (A_next - A) / 3 + 2, NP = NC + lag;
  const int As = producer ? A - sh : A;                   // this wave's first row ...
  const int nsteps = producer ? NP : NC;                  // ... and its steps
  const int R = i2.ring_rows;
  const int or_lo = A == 0 ? 0 : A + 2;
  int or_hi = A_next + 1;
  if (or_hi > out_last) or_hi = out_last;
  int deep = !no_clamp ? 0 : 8;
  const int colb = c0 + 3 * lane;
  // consumer: the strip-relative columns [lo, hi] it stores (see the single loop); a strip beyond the raster stores nothing
  StoreSide st(wout, g, c0, or_lo, or_hi);
  {
    const int lo = j == 0 ? (grp == 0 ? 0 : kGroupHaloL) : kHaloL;
    int hi = kStripIn - 1 - (j == 3 ? kGroupHaloR : kHaloR);
    if (hi > g.ncp - 1 - c0) hi = g.ncp - 1 - c0;
    st.any = hi >= lo;
    st.columns(st.any ? lo : 0, st.any ? hi : 0, lane);   // nothing to store: column 0 throughout
  }
  // producer: where its columns go in a ring row - its exact ones (and the group's outer halos); the others to the row's dump cells
  int dcol[3];
#pragma unroll
  for (int jj = 0; jj < 3; jj++) {
    const int cs = 3 * lane + jj;
    const bool own = cs >= (j == 0 ? 0 : kHaloL) && cs <= (j == 3 ? kStripIn - 1 : kStripIn - 1 - kHaloR);
    dcol[jj] = own ? kStripOut * j + cs : kGroupIn + jj;
  }
  const int rcol = kStripOut * j + 3 * lane;              // consumer: its first column in a ring row
  // The hand words through a pointer that says LDS: ds_read / ds_write in the wave's in-order LDS queue.  Through a generic pointer
  // they were FLAT operations, each volatile store followed by a wait for every global load and store of the wave in flight.
  volatile __attribute__((address_space(3))) int *const hand_v = (volatile __attribute__((address_space(3))) int *)hand;
  const int nb_lo = j > 0 ? j - 1 : 0, nb_hi = j < 3 ? j + 1 : 3;
  bool broken = false;
  // the smallest count of the (up to) three waves of the other role this one exchanges columns with, once it is >= need - or at once
  // where need <= 0
#ifdef WDPM_WAVE_TIMES
  unsigned wt_polls0 = 0, wt_polls1 = 0, wt_polls2 = 0, wt_ticks0 = 0, wt_ticks1 = 0, wt_ticks2 = 0, wt_waits = 0;
  int wt_phase = 0;
#endif
  auto await = [&](const int base, const int need) -> int {
    int m = 0, polls = 0;
#ifdef WDPM_WAVE_TIMES
    unsigned long long wt_a = 0;
#endif
    for (;;) {
      const int a = hand_v[base + nb_lo], b = hand_v[base + j], c = hand_v[base + nb_hi];
      m = a < b ? a : b;
      m = m < c ? m : c;
      m = __builtin_amdgcn_readfirstlane(m);
      if (m >= need || broken) break;
      if (++polls > kIter2Polls) {
        broken = true;
        if (lane == 0) *i2.err = 1u;
        break;
      }
#ifdef WDPM_WAVE_TIMES
      if (polls == 1) wt_a = wall_clock64();
#endif
      __builtin_amdgcn_s_sleep(2);
    }
#ifdef WDPM_WAVE_TIMES
    if (polls) {
      const unsigned dt = (unsigned)(wall_clock64() - wt_a);
      wt_waits++;
      if (wt_phase == 0) { wt_polls0 += polls; wt_ticks0 += dt; }
      else if (wt_phase == 1) { wt_polls1 += polls; wt_ticks1 += dt; }
      else { wt_polls2 += polls; wt_ticks2 += dt; }
    }
#endif
    asm volatile("" ::: "memory");
    return m;
  };
  // Strips beyond the raster's right edge (the last group rarely fills: at 16384^2 one strip of its four lies outside) retire at once
  // instead of marching on clamped loads: a consumer that stores nothing, a producer none of whose ring columns lies inside the raster.
  // Nothing stored depends on their columns - they lie beyond the border column, whose DEM is NODATA and lets nothing across (DESIGN 4.2,
  // tests/test_iter2_retired_strips.py) - but the neighbours read them: the producer leaves +0.0 in its columns of every ring row, so that
  // every ring cell holds a finite value, and either leaves a hand word no await() can exceed, written behind the zeros.
  const bool retire = producer ? c0 + (j == 0 ? 0 : kHaloL) >= g.ncp : !st.any;        // wave-uniform
  if (retire) {
    if (producer) {
      for (int r = 0; r < R; r++)
#pragma unroll
        for (int jj = 0; jj < 3; jj++) i2_ring[(size_t)r * kRingPitch + dcol[jj]] = 0.0;
      asm volatile("" ::: "memory");
    }
    hand_v[wave] = kIter2Retired;
    return;                                               // no barrier follows; no duration into the balance counters
  }
  const bool edge = (As + 3 * (nsteps + 1) > g.rows);
  double W[7][3], D[7][3];
#pragma unroll
  for (int k = 0; k < 7; k++)
#pragma unroll
    for (int jj = 0; jj < 3; jj++) { W[k][jj] = 0.0; D[k][jj] = WDPM_INF; }
  bool cdr[5];
#pragma unroll
  for (int k = 0; k < 5; k++) cdr[k] = false;
  DrainState ds;
  ds.td = 0.0;
  ds.hit = false;

  auto march = [&](auto edge_tag, auto role_tag) {
    constexpr bool EDGE = decltype(edge_tag)::value;
    constexpr bool PRODUCER = decltype(role_tag)::value;
    // a producer loads water and codes as the single loop does (WATER), a consumer the codes alone, its nine stores behind them
    const RowOffsets off(colb, g.ncp);
    auto prefetch = [&](Prefetched &P, const int r0) { prefetch_rows<DEM32, EDGE, PRODUCER>(P, r0, off, win, nullptr, code, g); };

    int put_slot = 0;                                      // producer: ring row of chunk row rr, rr = 0, 1, 2 ... as they are deposited
    int take_slot = 0;                                     // ring row of the next triple to take (triples never straddle the ring's end)
    // consumer: row triple t out of the ring, once the producers have deposited it (the last trip asks for one more than there is and drops it)
    auto take = [&](Prefetched &P, const int t) {
      const int need = t + lag + 1;
      await(0, need < NP ? need : NP);
      const double *row = i2_ring + (size_t)take_slot * kRingPitch + rcol;
      take_slot = take_slot + 3 >= R ? 0 : take_slot + 3;
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int jj = 0; jj < 3; jj++) P.NW[i][jj] = row[i * kRingPitch + jj];
      asm volatile("" ::: "memory");
      hand_v[4 + j] = t + 1;                              // carried out behind the reads
    };
    double staged[3][3];

    auto step = [&](const int n, Prefetched &P, auto nstages_tag) {
      constexpr int NSTAGES = decltype(nstages_tag)::value;
#ifdef WDPM_WAVE_TIMES
      wt_phase = n < 4 ? 0 : (n >= nsteps - 4 ? 2 : 1);
#endif
      if (!PRODUCER) st.read_staged(staged, stage_lds);
      decode_rows<DEM32, false>(W, D, P, code, 0.0);
      if (EDGE) mask_outside(W, D, As + 3 * n, colb, g);
      deep = deep_next(deep, W);
      prefetch(P, As + 3 * (n + 1));
      if (!PRODUCER) st.write_staged(staged, A + 3 * (n - 1) - 4);

      const int rbase = As + 3 * n - 4;
      if (deep) three_stages<0, false, NSTAGES, 1>(W, D, rbase, g.dr, cdr, ds);
      else three_stages<0, false, NSTAGES, 1 | 2>(W, D, rbase, g.dr, cdr, ds);
      // The next triple just in time: its latency is an LDS read, which the staging writes, the wait for the codes and the window
      // slide below cover.  Taken before the stages it kept nine doubles alive across them and asked the producers for their step
      // n + lag + 2 a step early - three rows of the ring's slack given away.
      if (!PRODUCER) take(P, n + 1);

      if (PRODUCER) {
        // rows rbase .. rbase + 2 are final: into the ring, once the consumers have taken what lies there (chunk rows < 0: nobody
        // reads them, the dump row)
        const int rr0 = 3 * n - 4 - sh;
        const int taken = await(4, n - sh / 3 - R / 3);
        if (i2.prio) {
          const int ahead = n - lag - taken;              // row triples deposited and not taken
          if (ahead <= 1) __builtin_amdgcn_s_setprio(3);  // the consumers are about to run dry: this wave first
          else if (ahead >= R / 3 - 1) __builtin_amdgcn_s_setprio(0);
          else __builtin_amdgcn_s_setprio(1);
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
          double *const row = i2_ring + (size_t)(rr0 + i >= 0 ? put_slot : R) * kRingPitch;
          if (rr0 + i >= 0) put_slot = put_slot + 1 >= R ? 0 : put_slot + 1;
#pragma unroll
          for (int jj = 0; jj < 3; jj++) row[dcol[jj]] = W[i][jj];
        }
        asm volatile("" ::: "memory");
        hand_v[j] = n + 1;                                // carried out behind the data
      } else {
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
          for (int jj = 0; jj < 3; jj++) stage_lds[i * kStripIn + 3 * lane + jj] = W[i][jj];
        __builtin_amdgcn_wave_barrier();
      }
      wait_rows<DEM32, PRODUCER, PRODUCER ? 0 : 9>(P);
      slide_window(W, D);
    };

    Prefetched P;
    if (!PRODUCER) take(P, 0);
    prefetch(P, As);
    wait_rows<DEM32, PRODUCER, 0>(P);
    step(0, P, std::integral_constant<int, 1>{});
    step(1, P, std::integral_constant<int, 2>{});
    for (int n = 2; n < nsteps; n++) step(n, P, std::integral_constant<int, 3>{});
    if (!PRODUCER) {
      st.read_staged(staged, stage_lds);
      st.write_staged(staged, A + 3 * (nsteps - 1) - 4);
    }
  };
  if (producer) {
    if (edge) march(std::true_type{}, std::true_type{});
    else march(std::false_type{}, std::true_type{});
  } else {
    if (edge) march(std::true_type{}, std::false_type{});
    else march(std::false_type{}, std::false_type{});
  }
  if (bal.acc && lane == 0) {
    const int x = chunk == i2.nchunks - 1 ? 8 : chunk == 0 ? 9 : (bal.rot ? xcc_phys : (int)(blockIdx.x & 7));
    if (!bal.rot || share == xcc_phys) {
      atomicAdd(bal.acc + x, wall_clock64() - bal_t0);
      atomicAdd(bal.acc + kBalClasses + x, 1ull);
    }
  }
#ifdef WDPM_WAVE_TIMES
  const int item = vb * 8 + wave;
  if (lane == 0 && item < 8192) {
    __builtin_amdgcn_s_waitcnt(0);
    g_wave_times[4 * item] = wt0;
    g_wave_times[4 * item + 1] = wall_clock64();
    g_wave_times[4 * item + 2] = __builtin_amdgcn_s_getreg((31 << 11) | 4) | ((unsigned long long)__builtin_amdgcn_s_getreg((3 << 11) | 20) << 32);
    g_wave_times[4 * item + 3] = ((unsigned long long)(4 * grp + j + (producer ? 0 : 0x4000)) << 48) | ((unsigned long long)(nsteps & 0xffff) << 32) | (unsigned)chunk;
    g_wave_waits[4 * item] = wt_polls0 | ((unsigned long long)wt_polls1 << 32);
    g_wave_waits[4 * item + 1] = wt_polls2 | ((unsigned long long)wt_waits << 32);
    g_wave_waits[4 * item + 2] = wt_ticks0 | ((unsigned long long)wt_ticks1 << 32);
    g_wave_waits[4 * item + 3] = wt_ticks2;
  }
#endif
}

/* DEM32: 0 = the fp64 DEM, 1 = verified 32-bit codes, 2 = those as 16-bit offsets + group bases (wdpm_kernels.h::DemCode) */
template <int MODULE, bool SZ_SAFE, int DEM32, bool FLUSH = false, bool MD = false, bool PLAIN = false>
__global__ void __launch_bounds__((fused_built_for<MODULE, SZ_SAFE, DEM32, MD>() >= 2 ? 512 : 256), (fused_built_for<MODULE, SZ_SAFE, DEM32, MD>()))
fused_iteration_kernel(const double *__restrict__ win, double *__restrict__ wout,
                       const double *__restrict__ dem, const DemCode code, const SlabGeom g, const int nstrips,
                       const int nitems, const int H, const int A0, const int out_last,
                       double *__restrict__ totaldrain, const double thres, const int drain_owed,
                       const TileFlags tf, const MaxDiffArgs md, const int prio, const int no_clamp, const BalanceArgs bal, const Iter2Args i2) {
  const int lane = threadIdx.x & 63;
  // Workgroups are dealt round-robin over the 8 XCDs (b and b+8 share an L2; placement is only a
  // speed matter, never correctness): give each XCD a contiguous run of work items so that the
  // halo columns shared by neighbouring strips hit in its L2 (+2 % measured).  gridDim.x is a
  // multiple of 8, so b -> (b % 8) * (gridDim.x / 8) + b / 8 is a permutation of the blocks.
  // ... and the share a workgroup takes is that of the PHYSICAL XCD it is expected to run on (BalanceArgs::rot): blockIdx % 8 turned by
  // the rotation the previous launch observed - one value for the whole launch, so this stays a permutation of the blocks.
  const int xcc_phys = (int)(__builtin_amdgcn_s_getreg((3 << 11) | 20) & 7);          // XCC_ID
  int rot_prev = 0;
  if (bal.rot) {
    rot_prev = __builtin_amdgcn_readfirstlane((int)(bal.rot[bal.parity] & 7));
    if (blockIdx.x == 0 && threadIdx.x == 0) bal.rot[bal.parity ^ 1] = (unsigned long long)xcc_phys;   // workgroup 0's XCD = this launch's rotation
  }
  const int share = (int)((blockIdx.x + (unsigned)rot_prev) % 8);
  const int vb = share * (gridDim.x / 8) + blockIdx.x / 8;
  // the wave number is the same in all 64 lanes: say so, and everything derived from it (strip,
  // chunk, row bases, loop bounds) lives in SGPRs and is computed on the scalar unit
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // A workgroup is eight waves where the launch puts two waves on every SIMD (one workgroup per CU: the two waves of a SIMD can
  // then see each other's progress in LDS - see `prio` in the marching loop), four where it leaves half of the slots empty.
  const int item = vb * (int)(blockDim.x >> 6) + wave;
  // Which two waves of this workgroup share a SIMD (see `prio` in the marching loop): settled by the waves themselves.
  // Rounds 3 - 4 took "SIMD id x 2 + the low bit of the wave slot" from HW_ID, which pairs two waves only while they sit in slots
  // that differ in bit 0 - true on an empty chip, not when other kernels hold slots (RCCL's send / recv kernels during the overlapped
  // iteration of an N-GPU run, the tail of the previous launch): slots 0 / 2 then share a word, each wave reads its own step
  // number back and the mechanism switches itself off.  Now every wave takes a seat at its SIMD (an LDS counter per SIMD id);
  // seats 0 and 1 of a SIMD are a pair, anything else (a SIMD with one or three of this workgroup's waves) runs without priorities.
  __shared__ int progress_all[8];                        // a pair's two step numbers: words 2 * SIMD + seat
  __shared__ int simd_seats[4];
  int my_word = 0;
  bool paired = false;
  if (prio) {                                            // the same in every wave of the launch: all of them reach the barriers
    if (threadIdx.x < 8) progress_all[threadIdx.x] = 0;
    if (threadIdx.x < 4) simd_seats[threadIdx.x] = 0;
    __syncthreads();
    const int simd = (int)((__builtin_amdgcn_s_getreg((31 << 11) | 4) >> 4) & 3);      // HW_ID: SIMD [5:4]
    int seat = 0;
    if (lane == 0) seat = atomicAdd(&simd_seats[simd], 1);
    seat = __builtin_amdgcn_readfirstlane(seat);
    __syncthreads();
    paired = seat < 2 && simd_seats[simd] == 2;
    my_word = 2 * simd + (seat & 1);
  }
  const int use_prio = paired ? 1 : 0;
  __shared__ double stage_all[8][3 * kStripIn];          // 4.5 KiB per wave, private to the wave
  if constexpr (MODULE == 0 && !SZ_SAFE && DEM32 != 0 && !FLUSH && !MD && PLAIN) {
    if (i2.on) {                                         // the same in every wave of the launch: two iterations (iter2_march)
      iter2_march<DEM32>(win, wout, code, g, H, out_last, no_clamp, bal, i2, vb, wave, lane, share, xcc_phys, stage_all[wave & 3]);
      return;
    }
  }
  if (item >= nitems) return;                       // wave-uniform
#ifdef WDPM_WAVE_TIMES
  const unsigned long long wt0 = wall_clock64();
#endif
  const int strip = item % nstrips, chunk = item / nstrips;
  const int c0 = kStripOut * strip;
  const int oc_lo = strip == 0 ? 0 : c0 + kHaloL;
  const int oc_hi = c0 + kStripIn - 1 - kHaloR;
  // a launch produces the rows [A0 + 2 (0 when A0 == 0), out_last] of the slab; A0 % 3 == 0
  int A = A0 + H * chunk, A_next = A + H;
  if (bal.table) {
    // chunk heights that follow what each XCD delivers (wdpm_kernels.h::BalanceArgs): this strip's own row boundaries.  Whatever
    // the table holds, no access can leave the slab: A is brought into it, waves near its end take the clamping loads
    // (`edge`), and rows outside [or_lo, or_hi] - or_hi never beyond out_last - are stored to the dump area.
    A = bal.table[chunk * nstrips + strip];
    A_next = bal.table[(chunk + 1) * nstrips + strip];
    A = A < 0 ? 0 : (A > g.rows ? g.rows : A);
    const int h = A_next - A;
    A_next = A + (h < 0 ? 0 : (h > 30000 ? 30000 : h));
  }
  const unsigned long long bal_t0 = bal.acc ? wall_clock64() : 0;
  const int nsteps = (A_next - A) / 3 + 2;
  const int or_lo = A == 0 ? 0 : A + 2;
  int or_hi = A_next + 1;
  if (or_hi > out_last) or_hi = out_last;

  // Dry tiles (wdpm_kernels.h::TileFlags): if this tile and its eight neighbours hold nothing but +0.0 in `win`,
  // the whole input window of this wave is dry - it lies inside those nine exact output blocks, because
  // H >= 6 and the halo is 8 / 13 columns - no centre has water to give, and the output block is all +0.0.
  // Then nothing is loaded, and nothing is stored either if `wout`'s block is known to hold zeros already.
  const int zpitch = nstrips + 2;                                      // flag arrays carry a border of 1s ("dry")
  const int tile = (chunk + 1) * zpitch + strip + 1;
  if (tf.zout) {                                                       // wave-uniform
    bool dry = false;
    if (tf.zin) {
      // nine unconditional loads in flight together (a bounds test per neighbour made nine dependent round trips)
      const unsigned char *z = tf.zin + tile;
      const unsigned f = z[-zpitch - 1] & z[-zpitch] & z[-zpitch + 1] & z[-1] & z[0] & z[1] & z[zpitch - 1] & z[zpitch] &
                         z[zpitch + 1];
      dry = f != 0;
    }
    if (dry) {
      if (!(tf.zout_known && tf.zout[tile] != 0)) {
        const int hi = oc_hi < g.ncp - 1 ? oc_hi : g.ncp - 1;
        for (int r = or_lo; r <= or_hi; r++)
#pragma unroll
          for (int k = 0; k < 3; k++) {
            const int c = oc_lo + 64 * k + lane;
            if (c <= hi) wout[(size_t)r * g.ncp + c] = 0.0;
          }
        if (lane == 0) tf.zout[tile] = 1;
      }
      return;
    }
  }
  unsigned long long nzmask = 0;        // lanes that staged a value other than 0.0 (no -0.0 exists where tiles are tracked)
  // CLAMP: which of the window's rows may hold a depth too large for the clamped neighbour step (see deep_next)
  int deep = (!SZ_SAFE && !no_clamp) ? 0 : 8;
  double md_max = 0.0;                  // MD: this lane's max |w - oldw| over the cells of its output block (WDPMCL.c:1239-1254)
  const int colb = c0 + 3 * lane;
  StoreSide st(wout, g, c0, or_lo, or_hi);
  st.columns(oc_lo - c0, (oc_hi < g.ncp - 1 ? oc_hi : g.ncp - 1) - c0, lane);
  double *const stage_lds = stage_all[wave];
  volatile int *const my_progress = progress_all + my_word;
  volatile int *const partner_progress = progress_all + (my_word ^ 1);
  bool cdr[5];
#pragma unroll
  for (int j = 0; j < 5; j++) cdr[j] = MODULE == 2 && colb + j == g.dc;
  DrainState ds;
  ds.td = MODULE == 2 ? *totaldrain : 0.0;
  ds.hit = false;
  // exactly one wave holds the outlet cell in its exact output region; it sees every pass that touches
  // the outlet, in the reference's order, so its totaldrain is the raster's
  bool owner = false;
  if (MODULE == 2) {
    const int dcol_hi = oc_hi < g.ncp - 1 ? oc_hi : g.ncp - 1;
    owner = g.dr >= or_lo && g.dr <= or_hi && g.dc >= oc_lo && g.dc <= dcol_hi;
    // drain_owed: the previous iteration's drain() (WDPMCL.c:1089 -> :1859-1897) has not been applied to `win`
    // yet - there is no launch of its own for it.  Its sum enters totaldrain here (row-major from 0.0, valid
    // cells with water, :1877-1884), its zeroing of the nine cells (:1885-1889) happens as rows are loaded.
    if (drain_owed && owner && g.dr >= 1 && g.dr <= g.rows - 2 && g.dc >= 1 && g.dc <= g.ncp - 2) ds.td = ds.td + owed_drain_sum(win, dem, g);
  }
  const bool owed_here = MODULE == 2 && drain_owed && g.dr >= 1 && g.dr <= g.rows - 2 && g.dc >= 1 && g.dc <= g.ncp - 2;
  bool owed_col[3];
#pragma unroll
  for (int j = 0; j < 3; j++) owed_col[j] = owed_here && colb + j >= g.dc - 1 && colb + j <= g.dc + 1;

  double W[7][3], D[7][3];
#pragma unroll
  for (int k = 0; k < 7; k++)
#pragma unroll
    for (int j = 0; j < 3; j++) { W[k][j] = 0.0; D[k][j] = WDPM_INF; }

  // Only waves of the last strip / last chunk can touch cells outside the slab; every other wave
  // loads without any predicate.  `edge` is wave-uniform (the margin lets interior waves prefetch
  // past their last step unconditionally).
  // Round 5: a strip that reaches past the raster's right edge is NOT an edge case.  Its lanes beyond column ncp - 1 hold whatever
  // the clamped loads bring - the border cell and the first cells of the next row - and never touch the raster: column ncp - 1 is the
  // reference's 1-cell border (bigdem = missingvalue, WDPMCL.c:796-807; +inf / NaN here), which neither gives (its centre test fails;
  // in the gate-free variants its depth is +0.0, or they would not run) nor receives (as a neighbour dem + w is inf / NaN and the
  // flow +-0), every path from a cell beyond the edge to a cell of the raster leads through it, and no lane beyond it is ever
  // stored (the store columns are clamped to the border, which holds what it held).  The kernel relied on that border before - it
  // runs centres on every column, the border's included.  Rounds 1 - 4 sent those waves down the masking instantiation of the
  // marching loop: one wave per workgroup, alone on a code path nobody shared its instruction-cache misses with - they ended 3.5 %
  // (8192^2 drain) to 12 % (the 8-GPU drain slab) after everybody else, the last waves of almost every launch
  // (profiles/r05/first_chunk_row.txt, wave_times_coledge.txt).
  const bool edge = (A + 3 * (nsteps + 1) > g.rows);
  const size_t pitch = (size_t)g.ncp;

  // The marching loop, instantiated for interior (EDGE = false) and edge waves.
  auto march = [&](auto edge_tag) {
    constexpr bool EDGE = decltype(edge_tag)::value;
    const RowOffsets off(colb, g.ncp);
    auto prefetch = [&](Prefetched &P, const int r0) { prefetch_rows<DEM32, EDGE, true>(P, r0, off, win, dem, code, g); };
    double staged[3][3];

    auto step = [&](const int n, Prefetched &P, auto nstages_tag) {
      constexpr int NSTAGES = decltype(nstages_tag)::value;
      int partner_at = 0;
      if (use_prio) {                                    // wave-uniform
        *my_progress = n;                                // every lane the same word
        partner_at = *partner_progress;                  // read back after the step's arithmetic
      }
      st.read_staged(staged, stage_lds);
      decode_rows<DEM32, FLUSH>(W, D, P, code, thres);
      if (MODULE == 2 && owed_here && A + 3 * n + 2 >= g.dr - 1 && A + 3 * n <= g.dr + 1) {   // wave-uniform, rare
#pragma unroll
        for (int i = 0; i < 3; i++) {
          const bool owed_row = A + 3 * n + i >= g.dr - 1 && A + 3 * n + i <= g.dr + 1;
#pragma unroll
          for (int j = 0; j < 3; j++) W[4 + i][j] = owed_row && owed_col[j] ? 0.0 : W[4 + i][j];
        }
      }
      if (EDGE) mask_outside(W, D, A + 3 * n, colb, g);
      if constexpr (!SZ_SAFE) deep = deep_next(deep, W);
      // always issued (the last trips re-read clamped / following rows and drop them)
      prefetch(P, A + 3 * (n + 1));
      // the rows the previous step staged in LDS go out now, behind the new loads and ahead of a
      // whole step of arithmetic (+1 % over storing at the end of the step); n = 0 has none: dump
      st.write_staged(staged, A + 3 * (n - 1) - 4);

      const int rbase = A + 3 * n - 4;                 // slab row of window slot 0
#ifndef WDPM_ABLATE_COMPUTE                            /* timing experiments only: memory pattern alone */
      if (SZ_SAFE || deep) three_stages<MODULE, SZ_SAFE, NSTAGES, (PLAIN ? 1 : 0)>(W, D, rbase, g.dr, cdr, ds);
      else three_stages<MODULE, SZ_SAFE, NSTAGES, (PLAIN ? 1 : 0) | 2>(W, D, rbase, g.dr, cdr, ds);
#else
#pragma unroll
      for (int j = 0; j < 3; j++) W[0][j] += D[0][j] + D[1][j] + D[2][j];   // keep the dem loads alive
#endif

      // rows 3n-4 .. 3n-2 have now seen all nine passes.  The wave transposes each row through its
      // private LDS slice (no barrier: a wave's LDS operations complete in order) so that every
      // store instruction writes 512 contiguous bytes; the stores themselves are issued by write_staged()
      // at the top of the next step.
      if (MD) {
        // rows 3n-4 .. 3n-2 are final: their part of the block's max-change reduction, against the snapshot
        // (which may still be owed the block's flush: applied as it is read).  Only cells of this wave's own
        // output block, of the rows asked for, with bigdem > missingvalue - plus the reference's seed cell [0][0].
        const int hi = oc_hi < g.ncp - 1 ? oc_hi : g.ncp - 1;
#pragma unroll
        for (int i = 0; i < 3; i++) {
          const int r = rbase + i;
          const bool row_in = r >= or_lo && r <= or_hi && r >= md.row_lo && r < md.row_hi;     // wave-uniform
          const int rc = r < 0 ? 0 : (r < g.rows ? r : g.rows - 1);
#pragma unroll
          for (int j = 0; j < 3; j++) {
            const int c = colb + j;
            const int cc = c < g.ncp ? c : g.ncp - 1;
            double o = md.old[(size_t)rc * pitch + cc];
            o = o < md.thres ? 0.0 : o;                                                         // :1059-1062
            const double dd = __builtin_fabs(W[i][j] - o);                                      // :1241
            const bool cell = row_in & (c >= oc_lo) & (c <= hi) & ((D[i][j] < WDPM_INF) | ((r == 0) & (c == 0)));
            md_max = (cell & (dd > md_max)) ? dd : md_max;                                        // :1245-1254
          }
        }
      }
      unsigned any_lo = 0, any_hi = 0;
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
          stage_lds[i * kStripIn + 3 * lane + j] = W[i][j];
          // "is any staged value something other than +0.0?": the OR of the nine bit images (v_or3_b32: nine instructions and one
          // compare per step, where a compare per value took twenty)
          any_lo |= (unsigned)__double2loint(W[i][j]);
          any_hi |= (unsigned)__double2hiint(W[i][j]);
        }
      nzmask |= __ballot(((any_lo | any_hi) != 0) & (colb < g.ncp));      // (lanes beyond the raster's right edge hold other rows' cells)
      __builtin_amdgcn_wave_barrier();
      if (use_prio) {
        const int p = __builtin_amdgcn_readfirstlane(partner_at);
        if (p > n) __builtin_amdgcn_s_setprio(3);        // the other wave of this SIMD is ahead: this one is served first
        else if (p < n) __builtin_amdgcn_s_setprio(0);
        else __builtin_amdgcn_s_setprio(1);
      }
      // The rows requested at the top of this step must have landed before the compiler may touch
      // their registers (it copies them around the loop back-edge): wait here, where the only
      // younger memory operations are the 9 stores issued right after them.
      wait_rows<DEM32, true, 9>(P);
      slide_window(W, D);
    };

    // The SIMD's arbiter serves the OLDER of its two waves first whenever both have an instruction ready.  Left alone, the older
    // wave of every SIMD gets ~65 % of the issue slots, finishes its chunk at 0.65 of the launch's time, and the younger runs
    // the last third alone with nobody to hide its latencies behind (tools/wave_times.py; 4096^2 in round 4: slot 0 ends at
    // 55.7 us, slot 1 at 85.2 us of a 90.4 us launch, wave-time in flight / (waves x span) = 0.77).
    // Round 3 answered with priorities that FALL as a wave advances through its chunk (four levels at fixed fractions, the
    // fractions different for the two slots, from a two-wave model of the arbiter): 0.96 in flight at 16384^2 (+5.6 %), but nothing
    // or a loss on chunks of fewer than ~40 steps - 4096^2, every 8-GPU slab - and an instantiation of its own.
    // Round 4: the two waves TELL each other where they are.  With two waves per SIMD a workgroup is eight waves, one workgroup
    // per CU, so the two waves of a SIMD share LDS: each step a wave writes its step number to its word (SIMD id x 2 + the
    // seat it took there at the start of the kernel) and reads the other's; whoever is behind gets priority 3, whoever is ahead 0,
    // level 1 when they are level (the older then leads by a step, and is overtaken).  Two LDS operations and a few scalar
    // instructions per step, no assumption about chunk heights or about who started first; a partner that has finished keeps its
    // last step number and reads as "ahead" until it is passed - either way only who issues first is decided here, never what is computed.
    // `prio` = 0 (WDPM_PRIO=0, or a launch of four-wave workgroups): no priorities.
    Prefetched P;
    prefetch(P, A);
    wait_rows<DEM32, true, 0>(P);
    // The dead stages of a chunk's first two steps are left out (see three_stages): 3 of 3 (H/3 + 2) stage executions.
    step(0, P, std::integral_constant<int, 1>{});      // nsteps >= 3: H >= 3
    step(1, P, std::integral_constant<int, 2>{});
    for (int n = 2; n < nsteps; n++) step(n, P, std::integral_constant<int, 3>{});
    st.read_staged(staged, stage_lds);
    st.write_staged(staged, A + 3 * (nsteps - 1) - 4);    // the last step's rows
  };
  if (edge) march(std::true_type{});
  else march(std::false_type{});

  if (MODULE == 2 && owner && lane == 0) *totaldrain = ds.td;
  if (MD) fold_max_diff(md_max, md, lane);
  if (tf.zout && lane == 0) {
    // every staged row went into the mask, the warm-up rows above the block included: a flag of 0 only says "unknown"
    tf.zout[tile] = nzmask ? 0 : 1;
    atomicAdd(tf.active, 1u);
  }
  if (bal.acc && lane == 0) {
    // class 0 .. 7: the XCD (workgroups are dealt round-robin over them); class 8: the waves of a strip's last chunk, whatever
    // their XCD - they take the clamping loads and the masks of the slab's lower edge on every step and end ~5 % late
    // (with `rot`: by physical XCD, and only where the share this workgroup took is the one sized for the XCD it ran on)
    const int x = chunk == tf.nchunks - 1 ? 8 : chunk == 0 ? 9 : (bal.rot ? xcc_phys : (int)(blockIdx.x & 7));
    if (!bal.rot || share == xcc_phys) {
      atomicAdd(bal.acc + x, wall_clock64() - bal_t0);
      atomicAdd(bal.acc + kBalClasses + x, 1ull);
    }
  }
#ifdef WDPM_WAVE_TIMES
  if (lane == 0 && item < 8192) {
    __builtin_amdgcn_s_waitcnt(0);   // the wave's stores have left
    g_wave_times[4 * item] = wt0;
    g_wave_times[4 * item + 1] = wall_clock64();
    g_wave_times[4 * item + 2] = __builtin_amdgcn_s_getreg((31 << 11) | 4) | ((unsigned long long)__builtin_amdgcn_s_getreg((3 << 11) | 20) << 32);  // HW_ID, XCC_ID
    g_wave_times[4 * item + 3] = ((unsigned long long)strip << 48) | ((unsigned long long)(nsteps & 0xffff) << 32) | (unsigned)chunk;   /* (the marching kernel) */
  }
#endif
}

/* wdpm_kernels.h::XcdBalance: (update) move the weights towards equal mean wave durations - weight 0 .. 7: the relative height of
 * the chunks whose work items run on that XCD (the physical one: BalanceArgs::rot), weight 8: a factor on a strip's last chunk (its
 * waves are the slab's lower edge and take the masking loop), weight 9: one on its first (round 5: the slab's first chunk row ends late);
 * `from_uniform`: the measured launches ran on equal heights, whatever the weights say - then rebuild the table of row boundaries
 * for the launch geometry given: per strip, heights in proportion to the weights of its chunks, in whole row triples, at least two
 * per chunk, the last boundary at the launch's last triple.  One workgroup; the sums are cleared for the next measurement. */
__global__ void __launch_bounds__(256)
xcd_rebalance_kernel(float *__restrict__ weight, unsigned long long *__restrict__ acc, int *__restrict__ table, const int nstrips,
                     const int nchunks, const int A0, const int out_last, const int ipx, const int update, const int from_uniform,
                     const int pair) {
  __shared__ float w[kBalClasses];
  if (threadIdx.x == 0) {
    float mean[kBalClasses], m = 0.f;
    bool all = true;
    for (int x = 0; x < kBalClasses; x++) {
      const float v = weight[x];
      w[x] = (v > 0.5f && v < 2.0f) ? v : 1.0f;
      const unsigned long long n = acc[kBalClasses + x];
      mean[x] = n ? (float)((double)acc[x] / (double)n) : 0.f;
      if (x < 8) { all = all && n > 0 && mean[x] > 0.f; m += mean[x]; }
    }
    if (update && all) {
      m *= 0.125f;
      float sum = 0.f;
      for (int x = 0; x < kBalClasses; x++) {
        if (x >= 8 && !(mean[x] > 0.f)) continue;            // (a launch of two chunk rows has no waves in a class of its own)
        const float base = from_uniform ? 1.0f : w[x];
        float r = m / mean[x];                               // > 1: these waves end early, they can take taller chunks
        r = r < 0.8f ? 0.8f : (r > 1.25f ? 1.25f : r);
        w[x] = base * (1.0f + 0.75f * (r - 1.0f));           // damped
        if (x < 8) sum += w[x];
      }
      for (int x = 0; x < 8; x++) {
        const float v = w[x] * 8.0f / sum;
        w[x] = v < 0.7f ? 0.7f : (v > 1.4f ? 1.4f : v);
      }
      for (int x = 8; x < kBalClasses; x++) w[x] = w[x] < 0.75f ? 0.75f : (w[x] > 1.2f ? 1.2f : w[x]);
    }
    for (int x = 0; x < kBalClasses; x++) { weight[x] = w[x]; acc[x] = 0; acc[kBalClasses + x] = 0; }
  }
  __syncthreads();
  const int T = (out_last - 1 - A0 + 2) / 3;                 // row triples the chunks of a strip share: A0 + 3 T >= out_last - 1
  auto wgt = [&](const int c, const int s) {
    const int x = (c * nstrips + s) / ipx;
    return w[x < 7 ? x : 7] * (c == nchunks - 1 ? w[8] : c == 0 ? w[9] : 1.0f);
  };
  for (int s = (int)threadIdx.x; s < nstrips; s += (int)blockDim.x) {
    float total = 0.f;
    for (int c = 0; c < nchunks; c++) total += wgt(c, s);
    float cum = 0.f;
    int prev = 0;
    table[s] = A0;
    // `pair` (round 5): heights come in whole row triples, so where a chunk is a few triples tall (an 8-GPU slab: 8.4) some chunks are
    // a triple taller than others - and a launch of one resident round ends with its busiest SIMD, i.e. with the pair of waves that
    // holds two tall chunks.  The two waves of a SIMD are waves w and w + 4 of an eight-wave workgroup, work items four apart: strips
    // s and s + 4 of one chunk row.  Rounding the boundaries of those two strips half a triple apart puts the tall chunks of one
    // beside the short chunks of the other (exactly so for equal weights: with a fractional height f <= 1/2 two tall chunks never
    // meet, with f > 1/2 two short ones never do), and every SIMD gets the same number of steps to within one.
    const float phase = pair ? (((s >> 2) & 1) ? 0.75f : 0.25f) : 0.5f;
    for (int c = 0; c < nchunks; c++) {
      cum += wgt(c, s);
      int t = c == nchunks - 1 ? T : (int)((float)T * cum / total + phase);
      const int lo = prev + 2, hi = T - 2 * (nchunks - 1 - c);
      t = t < lo ? lo : t;
      t = t > hi ? hi : t;
      table[(c + 1) * nstrips + s] = A0 + 3 * t;
      prev = t;
    }
  }
}

__global__ void dpp_probe_kernel(int *out) {
  const int lane = threadIdx.x;
  const double v = (double)lane;
  out[lane] = (int)lane_next(v);
  out[64 + lane] = (int)lane_prev(v, -2.0);
}

}  // namespace

static hipError_t dpp_selfcheck(hipStream_t s) {
  static std::atomic<int> state{0};   // 0 unknown, 1 ok, -1 bad; rank threads of one process launch concurrently: no plain statics
  if (state == 1) return hipSuccess;
  if (state == -1) return hipErrorUnknown;
  int *d = nullptr;
  int h[128];
  hipError_t e = hipMalloc(&d, sizeof h);
  if (e != hipSuccess) return e;
  WDPM_LEDGER(0, dpp_probe_kernel);
  hipLaunchKernelGGL(dpp_probe_kernel, dim3(1), dim3(64), 0, s, d);
  e = hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(d);
  if (e != hipSuccess) return e;
  bool ok = true;
  for (int l = 0; l < 64; l++) {
    ok = ok && h[l] == (l < 63 ? l + 1 : 0);
    ok = ok && h[64 + l] == (l > 0 ? l - 1 : -2);
  }
  state = ok ? 1 : -1;
  return ok ? hipSuccess : hipErrorUnknown;
}

using MarchingFn = decltype(&fused_iteration_kernel<0, false, 0, false, false, false>);
#define WDPM_ROW_MARCHING(...) WDPM_VARIANT_ROW(fused_iteration_kernel, __VA_ARGS__)
static const VariantRow<MarchingFn> kMarchingTable[] = {WDPM_VARIANTS_MARCHING(WDPM_ROW_MARCHING)};

/* DeviceFacts::resident_waves of one occupancy class, from the occupancy API */
template <int MODULE, bool SZ_SAFE, int DEM32>
static int resident_waves(const int cus) {
  int blocks = 2;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, fused_iteration_kernel<MODULE, SZ_SAFE, DEM32, false, false, false>, 256, 0) != hipSuccess || blocks < 1)
    blocks = 2;
  constexpr int built_for = fused_built_for<MODULE, SZ_SAFE, DEM32, false>();
  if (blocks > built_for) blocks = built_for;
  return cus * blocks * 4;
}

/* The facts of the calling thread's current device: queried when the first context on that device is created, never on the
 * launch path.  nullptr: no current device, or an ordinal beyond the table. */
const DeviceFacts *wdpm_device_facts() {
  constexpr int kMaxDevices = 64;
  static DeviceFacts facts[kMaxDevices];
  static std::once_flag once[kMaxDevices];      // rank threads create their contexts concurrently
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return nullptr;
  std::call_once(once[dev], [dev] {
    DeviceFacts &f = facts[dev];
    if (hipDeviceGetAttribute(&f.cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || f.cus < 1) f.cus = 256;
    if (hipDeviceGetAttribute(&f.lds_per_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess || f.lds_per_cu < 65536)
      f.lds_per_cu = 163840;
    f.resident_waves[0][0] = resident_waves<0, false, 0>(f.cus);
    f.resident_waves[0][1] = resident_waves<0, false, 1>(f.cus);
    f.resident_waves[0][2] = resident_waves<0, true, 0>(f.cus);
    f.resident_waves[1][0] = resident_waves<2, false, 0>(f.cus);
    f.resident_waves[1][1] = resident_waves<2, false, 1>(f.cus);
    f.resident_waves[1][2] = resident_waves<2, true, 0>(f.cus);
    wdpm_small_device_facts(&f);
  });
  return &facts[dev];
}

/* The tile-flag hand-over of a marching launch that keeps dry-tile flags (LaunchPlan::tiles_fit): what the kernel gets, and the
 * tiling the context's flags now stand for. */
static hipError_t tiles_hand_over(TilePlan *tiles, const LaunchPlan &p, hipStream_t s, TileFlags *tf) {
  // the flags describe one tiling: another chunk height or strip count makes the old ones meaningless
  const bool same = tiles->nstrips == p.nstrips && tiles->H == p.H && tiles->nchunks == p.nchunks;
  if (!same) {   /* new pitch: the output raster's flag array needs its border of 1s before the kernel fills the interior */
    const hipError_t e = hipMemsetAsync(tiles->zout, 1, (size_t)tiles->capacity, s);
    if (e != hipSuccess) return e;
  }
  tf->zin = same && tiles->zin_valid ? tiles->zin : nullptr;
  tf->zout = tiles->zout;
  tf->zout_known = same && tiles->zout_valid;
  tf->active = tiles->active;
  tiles->nstrips = p.nstrips; tiles->H = p.H; tiles->nchunks = p.nchunks;
  tiles->maintained = 1;
  return hipSuccess;
}

/* The balance bookkeeping of a marching launch that may look at the balance state (LaunchPlan::balance): rebuilds the table where
 * the geometry is new or three launches have been measured, keeps the measuring schedule, says what the kernel gets. */
static BalanceArgs balance_step(XcdBalance *bal, const LaunchRequest &q, const LaunchPlan &p, hipStream_t s) {
  BalanceArgs ba{nullptr, nullptr, nullptr, 0};
  if (p.table) {
    const bool same = bal->nstrips == p.nstrips && bal->nchunks == p.nchunks && bal->A0 == q.A0 && bal->out_last == q.out_last && bal->ipx == p.ipx;
    const bool update = bal->measured >= 3 && (same || bal->measured_uniform);
    if (!same || update) {
      WDPM_LEDGER(0, xcd_rebalance_kernel);
      hipLaunchKernelGGL(xcd_rebalance_kernel, dim3(1), dim3(256), 0, s, bal->weight, bal->acc, bal->table, p.nstrips, p.nchunks, q.A0,
                         q.out_last, p.ipx, update ? 1 : 0, bal->measured_uniform, p.pair);
      bal->measured_uniform = 0;
      bal->nstrips = p.nstrips; bal->nchunks = p.nchunks; bal->A0 = q.A0; bal->out_last = q.out_last; bal->ipx = p.ipx;
      bal->measured = 0;
      if (update) bal->updates++;
    }
    ba.table = bal->table;
    if (p.rot) {
      ba.rot = bal->acc + 2 * kBalClasses;          // shares and measurements by physical XCD (BalanceArgs::rot)
      ba.parity = bal->seq++ & 1;
    }
    // measured: while the weights are young, every steady launch (an update every three); afterwards three launches in 256
    if (p.steady && (bal->updates < 6 || (bal->launches & 255) < 3)) {
      if (bal->measured == 0 || !bal->measured_uniform) { ba.acc = bal->acc; bal->measured_uniform = 0; bal->measured++; }
    }
    bal->launches++;
  } else if (p.measure_equal && bal->updates == 0 && (bal->measured == 0 || bal->measured_uniform)) {
    // equal heights (a block that keeps dry-tile flags): what the XCDs deliver can be learnt here already
    ba.acc = bal->acc;
    ba.rot = bal->acc + 2 * kBalClasses;
    ba.parity = bal->seq++ & 1;
    bal->measured_uniform = 1;
    bal->measured++;
  }
  return ba;
}

/* queues what plan_iteration() decided for the request */
hipError_t wdpm_launch_iteration(const LaunchRequest &q, const LaunchPlan &p, const IterationBuffers &b) {
  if (b.tiles) b.tiles->maintained = 0;
  if (p.error) return hipErrorInvalidValue;
  hipError_t e = dpp_selfcheck(b.stream);
  if (e != hipSuccess) return e;
  if (p.family != WDPM_FAMILY_MARCHING) return wdpm_launch_small(q, p, b);
  const int at = wdpm_find_variant(kMarchingVariants, p.targs);
  if (at < 0) return hipErrorInvalidValue;
  TileFlags tf{nullptr, nullptr, 0, nullptr, p.nchunks};
  if (p.tiles_fit) {
    e = tiles_hand_over(b.tiles, p, b.stream, &tf);
    if (e != hipSuccess) return e;
  }
  const MaxDiffArgs mda = p.fold_md ? *b.md : MaxDiffArgs{nullptr, 0.0, 0, 0, nullptr};
  if (p.fold_md) tf = TileFlags{nullptr, nullptr, 0, nullptr, p.nchunks};   /* every wave must look at its block: no skipping in this launch */
  if (p.fold_md && b.tiles) b.tiles->maintained = 0;
  const BalanceArgs ba = p.balance ? balance_step(b.bal, q, p, b.stream) : BalanceArgs{nullptr, nullptr, nullptr, 0};
  if (p.iter2 && !b.iter2_err) return hipErrorInvalidValue;
  const Iter2Args i2{p.iter2, p.nstrips, p.nchunks, p.ring_rows, p.iter2_prio, b.iter2_err};
  wdpm_ledger_count(*kMarchingTable[at].slot, p.ledger_sw);
  hipLaunchKernelGGL(kMarchingTable[at].fn, dim3(p.grid), dim3(p.block), p.lds, b.stream, b.w_in, b.w_out, b.dem, *b.code, q.g, p.nstrips, p.nitems,
                     p.H, q.A0, q.out_last, b.totaldrain, b.thres, q.module == 2 ? b.drain_owed : 0, tf, mda, p.prio, p.no_clamp, ba, i2);
  return hipGetLastError();
}

#ifdef WDPM_WAVE_TIMES
extern "C" int wdpm_debug_wave_times(unsigned long long *out, int nwaves) {
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_times), (size_t)nwaves * 32) != hipSuccess;
}
extern "C" int wdpm_debug_wave_waits(unsigned long long *out, int nwaves) {
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_waits), (size_t)nwaves * 32) != hipSuccess;
}
#endif
