/*
 * wdpm_iteration.h — what the three iteration kernels share: one whole WDPM iteration (all 9 colour passes, reference
 * src/WDPMCL.c:1094-1106, kernels runoff.cl:137-183) in ONE launch.  The marching kernel is wdpm_march.hip, the triangle and relay
 * kernels of small rasters are wdpm_small.hip; a function is here only if both units call it.  DESIGN.md §4 has the derivation, and
 * tests/fused_model.py checks the schedule against the oracle.
 *
 *  - A wave64 is the unit of work.  Lane m owns raster columns c0+3m .. c0+3m+2, so a wave covers a 192-column strip and a
 *    64-lane row load is one contiguous 1536-byte segment.
 *  - A 3x3 block of pass (oi,oj) only needs its nine cells to have finished all earlier passes, so row alignment oi=1 may run on
 *    rows 3n..3n+2, then oi=2 on rows 3n-2..3n, then oi=3 on rows 3n-4..3n-2: a skew that respects every dependency of the
 *    reference's pass order (block_update is one block, stage_impl one row alignment).
 *  - Within a row alignment the three column alignments oj=1,2,3 shift the blocks right by one
 *    column each: the lane borrows column 0 (then column 1) of lane m+1 with a DPP wave_shl:1
 *    register move, updates it, and hands both back with wave_shr:1.  No LDS traffic.
 *  - Information moves at most 8 columns left / 12 right and 2 rows up / 4 down per iteration, so
 *    a wave's 192 x (H+6) input trapezoid yields a 171 x H exact output; neighbouring waves
 *    recompute the overlap (redundant, bit-identical work) instead of communicating.
 *  - Cells with bigdem <= missingvalue and cells outside the slab are held as dem = +inf: as a
 *    neighbour this makes ht_diff -inf/NaN, so `ht_diff > 0` is false with no extra test
 *    (WDPMCL.c:1944); as a centre the gate `dem < +inf` replaces `bigdem > missingvalue` (:1099).
 *
 * Results are bit-identical to the serial reference: same operands, same order, fp64, no FMA in
 * the stencil (the DEM decode uses two, on values it has been verified to reproduce exactly).
 *
 * Three kernels share the per-block arithmetic and the trapezoid:
 *   fused_iteration_kernel  the marching window: rasters that fill the chip (from ~2300^2 add, ~2900^2 drain)
 *   relay_iteration_kernel  workgroups of four / eight waves, one row block per wave and row alignment, shared rows passed
 *                           through LDS: small and mid-size rasters (round 3; 482^2 add 7.3 -> 5.2 us, drain 12.1 -> 8.4)
 *   tri_iteration_kernel    one wave, nine (twelve) rows in, three (six) out, row blocks in lockstep: what is between the two,
 *                           and a small raster's last launch of a block (max diff folded in)
 * owed_drain_sum, fold_max_diff and any_above_3m serve all three.
 * plan_iteration (wdpm_dispatch.h) picks by size, module and what is known about the raster.
 */
#ifndef WDPM_ITERATION_H
#define WDPM_ITERATION_H

#include "wdpm_kernels.h"
#include "wdpm_ledger.h"
#include "wdpm_stencil.h"

namespace {

/* strip geometry (kLanes, kStripIn, kHaloL / kHaloR, kStripOut): wdpm_dispatch.h, which sizes the launches by it */

#define WDPM_INF (__builtin_inf())

/* value held by lane+1; lane 63 receives 0.0 (DPP bound_ctrl zero fill, so no register has to
 * be preset).  v_mov_b32_dpp wave_shl:1.  Lane 63's borrowed columns lie beyond the strip: its
 * blocks of passes oj=2,3 are inside the right halo whose results are never stored, so
 * any finite fill is as good as the true value there. */
__device__ __forceinline__ double lane_next(const double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, 0x130, 0xF, 0xF, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, 0x130, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

/* value held by lane-1; lane 0 keeps `keep`.  v_mov_b32_dpp wave_shr:1 */
__device__ __forceinline__ double lane_prev(const double v, const double keep) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(__double2loint(keep), lo, 0x138, 0xF, 0xF, false);
  hi = __builtin_amdgcn_update_dpp(__double2hiint(keep), hi, 0x138, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double wave_read(const double v, const int src_lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
  return __hiloint2double(hi, lo);
}

/* drain-module bookkeeping carried through the passes (compiles away for add/subtract) */
struct DrainState {
  double td;      // running totaldrain (wave-uniform value, one copy per lane)
  bool hit;       // this lane drained in the current pass
};

/* one neighbour step of runoffd() including its outlet branch (WDPMCL.c:1975-2002) */
__device__ __forceinline__ void step_drain(const double dc, double &wc, const double dn, double &wn,
                                           const bool gate, const bool is_outlet, DrainState &ds) {
  const bool hit = gate & is_outlet & (dn < WDPM_INF);   // :1976,1980
  const double td2 = (ds.td + wn) + wc;                   // :1982
  ds.td = hit ? td2 : ds.td;
  ds.hit = ds.hit | hit;
  wn = hit ? 0.0 : wn;                                    // :1983
  wc = hit ? 0.0 : wc;                                    // :1984
  flow_drain(dc, wc, dn, wn, gate & !hit);                // :1988-2000
}

/* one 3x3 block of one colour pass: centre (1,1), neighbours in row-major order.  OUTLET (drain
 * only): this block may touch the outlet cell, run runoffd()'s outlet branch too; the caller knows
 * wave-uniformly that it cannot for all but a handful of the raster's blocks. */
/* PLAIN (only with !SZ_SAFE): the caller knows that every cell which may not give water - dry, NODATA, outside the slab - holds
 * +0.0 exactly (wdpm_kernels.h::wdpm_launch_scan_water; no operation of the loop leaves that state).  The centre test of the
 * sweep (WDPMCL.c:1099) then costs nothing: for a centre depth of +0.0 the neighbour steps below come out as f = +-0 by
 * themselves, whatever the elevations - finite centre: dem_c > en gives x = w_c = 0, otherwise ht = dem_c - en <= 0 and
 * max(ht / 8, -0.0) = +-0; NODATA centre (dem = +inf): inf > en gives x = w_c = 0, and next to a NODATA neighbour ht is NaN,
 * which v_max turns into -0.0 - and w + (+-0) == w, w - |+-0| == w for every w that is not -0.0.  (drain: the same through
 * min(max(x / 8, -0.0), w_c = 0).)  Four instructions per block less for add, eight for drain. */
/* FLAGS: bit 0 = PLAIN, bit 1 = CLAMP (wdpm_stencil.h::eighth_clamped: the caller knows that no depth of this block exceeds 8 m
 * during the pass - see `deep` in the marching kernel; never on the outlet's path) */
template <int MODULE, bool SZ_SAFE, bool OUTLET = true, int FLAGS = 0>
__device__ __forceinline__ void block_update(
    double &w00, double &w01, double &w02, double &w10, double &w11, double &w12, double &w20, double &w21,
    double &w22, const double d00, const double d01, const double d02, const double d10, const double d11,
    const double d12, const double d20, const double d21, const double d22,
    const bool rd0, const bool rd1, const bool rd2, const bool cd0, const bool cd1, const bool cd2,
    DrainState &ds) {
  constexpr bool PLAIN = (FLAGS & 1) != 0, CL = (FLAGS & 2) != 0;
  double wc = w11;
  bool gate = (wc > 0.0) & (d11 < WDPM_INF);            // WDPMCL.c:1099
  if (MODULE == 2 && !OUTLET && !SZ_SAFE && PLAIN) {
    flow_drain_nz<CL>(d11, wc, d00, w00);
    flow_drain_nz<CL>(d11, wc, d01, w01);
    flow_drain_nz<CL>(d11, wc, d02, w02);
    flow_drain_nz<CL>(d11, wc, d10, w10);
    flow_drain_nz<CL>(d11, wc, d12, w12);
    flow_drain_nz<CL>(d11, wc, d20, w20);
    flow_drain_nz<CL>(d11, wc, d21, w21);
    flow_drain_nz<CL>(d11, wc, d22, w22);
  } else if (MODULE == 2 && !OUTLET && !SZ_SAFE) {
    const double dce = gate ? d11 : -WDPM_INF;           // see flow_drain_nz
    wc = gate ? wc : 0.0;                                // its clamp needs a centre depth >= +0
    flow_drain_nz<CL>(dce, wc, d00, w00);
    flow_drain_nz<CL>(dce, wc, d01, w01);
    flow_drain_nz<CL>(dce, wc, d02, w02);
    flow_drain_nz<CL>(dce, wc, d10, w10);
    flow_drain_nz<CL>(dce, wc, d12, w12);
    flow_drain_nz<CL>(dce, wc, d20, w20);
    flow_drain_nz<CL>(dce, wc, d21, w21);
    flow_drain_nz<CL>(dce, wc, d22, w22);
    wc = gate ? wc : w11;
  } else if (MODULE == 2 && !OUTLET) {
    flow_drain(d11, wc, d00, w00, gate);
    flow_drain(d11, wc, d01, w01, gate);
    flow_drain(d11, wc, d02, w02, gate);
    flow_drain(d11, wc, d10, w10, gate);
    flow_drain(d11, wc, d12, w12, gate);
    flow_drain(d11, wc, d20, w20, gate);
    flow_drain(d11, wc, d21, w21, gate);
    flow_drain(d11, wc, d22, w22, gate);
  } else if (MODULE == 2 && !SZ_SAFE) {
    // A block that may hold the outlet, no -0.0 in the raster: the plain neighbour step (flow_drain_nz) plus,
    // for the ONE neighbour position that can be the outlet in this wave, runoffd()'s sink (:1980-1985).
    // Which of the block's rows is the outlet's row is wave-uniform (rd*), whether ANY lane has the outlet's
    // column at block column c takes a ballot (anyc*): the sink's few instructions sit behind a scalar branch
    // that all but a handful of the raster's blocks never take.  After the sink the centre holds 0, and a
    // centre without water moves nothing in the remaining steps (f = min(.., 0)), exactly as in the reference,
    // whose loop also runs on with w[centre] = 0.
    gate = gate & !(rd1 & cd1);                          // :1082 the outlet is never a centre
    const double dce = gate ? d11 : -WDPM_INF;
    wc = gate ? wc : 0.0;
    const bool any0 = __ballot(cd0) != 0, any1 = __ballot(cd1) != 0, any2 = __ballot(cd2) != 0;
    bool hit_any = false;
    auto nb = [&](const double dn, double &wn, const bool rd, const bool anyc, const bool cd) {
      if (rd & anyc) {                                   // wave-uniform
        const bool hit = gate & cd & (dn < WDPM_INF);    // :1976,1980
        const double td2 = (ds.td + wn) + wc;            // :1982
        ds.td = hit ? td2 : ds.td;
        wn = hit ? 0.0 : wn;                             // :1983
        wc = hit ? 0.0 : wc;                             // :1984
        hit_any = hit_any | hit;
      }
      flow_drain_nz<false>(dce, wc, dn, wn);                 // :1988-2000 (never clamped: the outlet's path is off the hot path)
    };
    nb(d00, w00, rd0, any0, cd0);
    nb(d01, w01, rd0, any1, cd1);
    nb(d02, w02, rd0, any2, cd2);
    nb(d10, w10, rd1, any0, cd0);
    nb(d12, w12, rd1, any2, cd2);
    nb(d20, w20, rd2, any0, cd0);
    nb(d21, w21, rd2, any1, cd1);
    nb(d22, w22, rd2, any2, cd2);
    wc = gate ? wc : w11;
    // at most one lane of the wave holds the outlet in this pass: make its totaldrain the wave's
    const unsigned long long m = __ballot(hit_any);
    if (m) ds.td = wave_read(ds.td, __ffsll((long long)m) - 1);
  } else if (MODULE == 2) {
    gate = gate & !(rd1 & cd1);                          // :1082 the outlet is never a centre
    ds.hit = false;
    step_drain(d11, wc, d00, w00, gate, rd0 & cd0, ds);
    step_drain(d11, wc, d01, w01, gate, rd0 & cd1, ds);
    step_drain(d11, wc, d02, w02, gate, rd0 & cd2, ds);
    step_drain(d11, wc, d10, w10, gate, rd1 & cd0, ds);
    step_drain(d11, wc, d12, w12, gate, rd1 & cd2, ds);
    step_drain(d11, wc, d20, w20, gate, rd2 & cd0, ds);
    step_drain(d11, wc, d21, w21, gate, rd2 & cd1, ds);
    step_drain(d11, wc, d22, w22, gate, rd2 & cd2, ds);
    // at most one lane of the wave holds the outlet in this pass: make its totaldrain the wave's
    const unsigned long long m = __ballot(ds.hit);
    if (m) ds.td = wave_read(ds.td, __ffsll((long long)m) - 1);
  } else if (!SZ_SAFE) {
    // no -0.0 in the raster: the gate rides on the centre elevation (see flow_add_nz) - or is not needed at all (PLAIN)
    const double dce = PLAIN ? d11 : (gate ? d11 : -WDPM_INF);
    flow_add_nz<CL>(dce, wc, d00, w00);
    flow_add_nz<CL>(dce, wc, d01, w01);
    flow_add_nz<CL>(dce, wc, d02, w02);
    flow_add_nz<CL>(dce, wc, d10, w10);
    flow_add_nz<CL>(dce, wc, d12, w12);
    flow_add_nz<CL>(dce, wc, d20, w20);
    flow_add_nz<CL>(dce, wc, d21, w21);
    flow_add_nz<CL>(dce, wc, d22, w22);
  } else {
    flow_add(d11, wc, d00, w00, gate);
    flow_add(d11, wc, d01, w01, gate);
    flow_add(d11, wc, d02, w02, gate);
    flow_add(d11, wc, d10, w10, gate);
    flow_add(d11, wc, d12, w12, gate);
    flow_add(d11, wc, d20, w20, gate);
    flow_add(d11, wc, d21, w21, gate);
    flow_add(d11, wc, d22, w22, gate);
  }
  w11 = wc;
}

/* the three column alignments oj = 1,2,3 of one row alignment, on window slots S0..S0+2 */
template <int MODULE, bool SZ_SAFE, int S0, bool OUTLET, int PLAIN = 0>
__device__ __forceinline__ void stage_impl(double (&W)[7][3], const double (&D)[7][3], const int row_s0,
                                           const int drain_row, const bool (&cdr)[5], DrainState &ds) {
  const bool rd0 = MODULE == 2 && OUTLET && row_s0 == drain_row;
  const bool rd1 = MODULE == 2 && OUTLET && row_s0 + 1 == drain_row;
  const bool rd2 = MODULE == 2 && OUTLET && row_s0 + 2 == drain_row;
  constexpr int a = S0, b = S0 + 1, c = S0 + 2;
  // oj = 1: own columns 0,1,2
  block_update<MODULE, SZ_SAFE, OUTLET, PLAIN>(W[a][0], W[a][1], W[a][2], W[b][0], W[b][1], W[b][2], W[c][0], W[c][1], W[c][2],
                       D[a][0], D[a][1], D[a][2], D[b][0], D[b][1], D[b][2], D[c][0], D[c][1], D[c][2],
                       rd0, rd1, rd2, cdr[0], cdr[1], cdr[2], ds);
  // oj = 2: own columns 1,2 + column 0 of the next lane
  double wa0 = lane_next(W[a][0]), wb0 = lane_next(W[b][0]), wc0 = lane_next(W[c][0]);
  const double da0 = lane_next(D[a][0]), db0 = lane_next(D[b][0]),
               dc0 = lane_next(D[c][0]);
  block_update<MODULE, SZ_SAFE, OUTLET, PLAIN>(W[a][1], W[a][2], wa0, W[b][1], W[b][2], wb0, W[c][1], W[c][2], wc0,
                       D[a][1], D[a][2], da0, D[b][1], D[b][2], db0, D[c][1], D[c][2], dc0,
                       rd0, rd1, rd2, cdr[1], cdr[2], cdr[3], ds);
  // oj = 3: own column 2 + columns 0,1 of the next lane
  double wa1 = lane_next(W[a][1]), wb1 = lane_next(W[b][1]), wc1 = lane_next(W[c][1]);
  const double da1 = lane_next(D[a][1]), db1 = lane_next(D[b][1]),
               dc1 = lane_next(D[c][1]);
  block_update<MODULE, SZ_SAFE, OUTLET, PLAIN>(W[a][2], wa0, wa1, W[b][2], wb0, wb1, W[c][2], wc0, wc1,
                       D[a][2], da0, da1, D[b][2], db0, db1, D[c][2], dc0, dc1,
                       rd0, rd1, rd2, cdr[2], cdr[3], cdr[4], ds);
  // hand the borrowed columns back to lane+1; lane 0 keeps its own (nothing to its left)
  W[a][0] = lane_prev(wa0, W[a][0]);  W[a][1] = lane_prev(wa1, W[a][1]);
  W[b][0] = lane_prev(wb0, W[b][0]);  W[b][1] = lane_prev(wb1, W[b][1]);
  W[c][0] = lane_prev(wc0, W[c][0]);  W[c][1] = lane_prev(wc1, W[c][1]);
}

/* "does any lane hold a depth above 3 m in these three rows?" - the high words of the nine values compared as integers: a negative
 * or NaN depth counts as deep.  Wave-uniform. */
__device__ __forceinline__ bool any_above_3m(const double (*w)[3]) {
  auto hi = [](const double v) { return (unsigned)__double2hiint(v); };
  auto max3 = [](const unsigned a, const unsigned b, const unsigned c) { const unsigned m = a > b ? a : b; return m > c ? m : c; };
  unsigned hm = max3(hi(w[0][0]), hi(w[0][1]), hi(w[0][2]));
  hm = max3(hm, hi(w[1][0]), hi(w[1][1]));
  hm = max3(hm, hi(w[1][2]), hi(w[2][0]));
  hm = max3(hm, hi(w[2][1]), hi(w[2][2]));
  return __ballot(hm > 0x40080000u) != 0;               // 0x40080000'00000000 = 3.0
}

/* Drain: the sum the previous iteration's drain() (WDPMCL.c:1089 -> :1859-1897) owes to totaldrain - the outlet's 3x3, row-major
 * from 0.0, valid cells with water (:1877-1884).  The caller knows that the outlet lies inside the slab's border. */
__device__ __forceinline__ double owed_drain_sum(const double *__restrict__ win, const double *__restrict__ dem, const SlabGeom g) {
  double sum = 0.0;
#pragma unroll
  for (int i = -1; i <= 1; i++)
#pragma unroll
    for (int j = -1; j <= 1; j++) {
      const size_t k = (size_t)(g.dr + i) * g.ncp + (g.dc + j);
      const double wk = win[k];
      if (dem[k] < WDPM_INF && wk > 0) sum += wk;
    }
  return sum;
}

/* MD: the lanes' max |w - oldw| folded over the wave, one atomicMax per wave on the uint64 image (>= 0: order-preserving) */
__device__ __forceinline__ void fold_max_diff(double md_max, const MaxDiffArgs &md, const int lane) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double o = __shfl_xor(md_max, off, 64);
    md_max = o > md_max ? o : md_max;
  }
  if (lane == 0 && md_max > 0.0) atomicMax(md.bits, (unsigned long long)__double_as_longlong(md_max));
}

}  // namespace

/* One row of a family's launch table: the template arguments, the instantiation, its ledger slot.  Every instantiation of a family
 * has the family's one signature (a row of another type does not compile); the tables are made from the variant lists of
 * wdpm_dispatch.h and from nothing else, so those lists are also what the device code and the ledger contain. */
template <class Fn> struct VariantRow { int targs[6]; Fn fn; const int *slot; };
#define WDPM_VARIANT_ROW(KERNEL, ...) {{__VA_ARGS__}, &KERNEL<__VA_ARGS__>, &WdpmLedgerSlot<&KERNEL<__VA_ARGS__>, __VA_ARGS__>::slot},

#endif /* WDPM_ITERATION_H */
